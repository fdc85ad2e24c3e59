"""Host side of the prediction path (UNet.predict, cmunet_amd.infer): argument checks and structure inference, no GPU needed."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_predict_has_no_cpu_fallback_and_checks_its_arguments():
    from cmunet_amd.model import UNet
    m = UNet(base_ch=8, depth=3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.predict(torch.zeros(1, 16, 16))
    for t in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="threshold"):
            m.predict(torch.zeros(1, 16, 16), threshold=t)
    with pytest.raises(ValueError, match=r"\(B,H,W\)"):
        m.predict(torch.zeros(1, 1, 16, 16))
    with pytest.raises(ValueError, match="prob_class"):
        m.predict(torch.zeros(1, 16, 16), prob_class=2)
    assert m.training      # nothing above flipped the mode


@pytest.mark.parametrize("geom", [(2, 16, 3), (1, 8, 3), (3, 8, 4)])
def test_load_segmentation_model_infers_the_structure(geom):
    from cmunet_amd import infer
    from cmunet_amd.model import UNet
    K, base, depth = geom
    src = UNet(out_classes=K, base_ch=base, depth=depth)
    sd = src.state_dict()
    assert infer._unet_geometry(sd) == geom
    m = infer.load_segmentation_model(sd, device="cpu")
    assert not m.training and list(m.state_dict()) == list(sd)
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), sd.values()))
    assert infer.load_segmentation_model({"state_dict": sd}, dtype="f16", device="cpu").dtype == "f16"
    with pytest.raises(ValueError, match="conv_last.weight"):
        infer.load_segmentation_model({"foo": torch.zeros(1)}, device="cpu")


def test_load_segmentation_model_reads_both_file_forms(tmp_path):
    from cmunet_amd import infer
    from cmunet_amd.model import UNet
    src = UNet(out_classes=1, base_ch=8, depth=3, dtype="f16")
    torch.save(src, tmp_path / "best_model.pth")
    torch.save(src.state_dict(), tmp_path / "state.pth")
    for name in ("best_model.pth", "state.pth"):
        m = infer.load_segmentation_model(str(tmp_path / name), dtype="bf16", device="cpu")
        assert isinstance(m, UNet) and not m.training
        assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), src.state_dict().values()))
        assert {mod.dtype for mod in m.modules() if hasattr(mod, "dtype")} == {"bf16"}     # the run's storage type, on every block


def test_segmenter_checks_its_size_against_the_depth():
    from cmunet_amd import infer
    from cmunet_amd.model import UNet
    net = UNet(base_ch=4, depth=5)
    with pytest.raises(ValueError, match="multiple of 16"):
        infer.Segmenter(net, size=250)
    infer.Segmenter(net, size=256)
    infer.Segmenter(net, size=None)
    with pytest.raises(ValueError, match="threshold"):
        infer.Segmenter(net, threshold=1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        infer.Segmenter(net, size=None).segment([torch.zeros(16, 16)])


def test_cli_help_runs_in_a_fresh_process():
    r = subprocess.run([sys.executable, "-m", "cmunet_amd.infer", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    for flag in ("--model", "--images", "--out", "--size", "--batch", "--dtype", "--threshold"):
        assert flag in r.stdout
