"""The whole GCRN prior with the chunked LSTM form switched on (nets.GcrnPlan.chunk_proj) against the committed GCRN goldens at
the tolerance tests/test_gpu_parity.py: test_gcrn_golden holds the shipped form to: T = 401 (13 chunks, the last of 17 frames)
in the chunked form, and T = 20 with TC lowered to 8 (three chunks, the last of 4 frames).  At the shipped TC = 32 a plan of
fewer than 64 frames keeps the three-stage wavefront."""
import pytest
import torch

from conftest import golden, pkg, rel_l2, seeded

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def test_gcrn_golden_with_the_chunked_form(weights, monkeypatch):
    import __graft_entry__ as ge

    ge.build()
    pkg("_lib").load()
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    monkeypatch.setattr(pkg("nets").GcrnPlan, "chunk_proj", True)
    assert not pkg("nets").GcrnPlan(pkg("nets").Ctx(DEV), weights("GCRN"), 2, 63).chunk      # T < 2 TC
    g = golden("gcrn_t401")
    op = pkg("ops").GCRNOp(weights("GCRN"), DEV)
    out = op(seeded((1, 2, 401, 161), g["seed_x"]).to(DEV)).cpu()
    net = op._plans[(1, 401)]
    assert net.chunk and net.hT.shape[0] == 2 * net.CHUNK_TC == 64
    assert rel_l2(out[0, :, ::16, :], g["rows"]) < 5e-5
    monkeypatch.setattr(pkg("nets").GcrnPlan, "CHUNK_TC", 8)
    g = golden("gcrn_small")
    op = pkg("ops").GCRNOp(weights("GCRN"), DEV)
    out = op(seeded((2, 2, 20, 161), g["seed_x"]).to(DEV))
    net = op._plans[(2, 20)]
    torch.cuda.synchronize()
    assert net.chunk and net.hT.shape[0] == 16
    assert rel_l2(net.glstm_out().cpu(), g["glstm"]) < 2e-5
    assert rel_l2(out.cpu(), g["out"]) < 2e-5
