"""CPU: the host side of exact ragged batches for the DB-AIAT priors - the argument check with ``masked``, the descriptors
that carry the new length tables, the refusals that did not change and the command-line flag."""
import ctypes as C

import pytest

from conftest import pkg

AIA_PRIORS = ("aia_complex_trans_ri", "dual_aia_trans_merge_crm")


def test_ragged_args_takes_the_db_aiat_priors_only_when_masked():
    pl = pkg("pipeline")
    for prior in AIA_PRIORS:
        pl.ragged_args(prior, 16000, masked=True)
        pl.ragged_args(prior, 16000, True)                      # the third positional argument
        with pytest.raises(ValueError, match="bidirectional GRU"):
            pl.ragged_args(prior, 16000, masked=False)
        with pytest.raises(ValueError, match="bidirectional GRU"):
            pl.ragged_args(prior, 16000)
        with pytest.raises(ValueError, match="L_"):
            pl.ragged_args(prior, None, masked=True)            # the masked plan needs the signal front / back end too
    for prior in ("GCRN", "DiffUNet"):
        pl.ragged_args(prior, 16000, masked=True)               # the flag changes nothing for the other priors
    with pytest.raises(ValueError):
        pl.ragged_args("no_such_prior", 16000, masked=True)


def test_pipeline_refuses_without_the_option():
    pl = pkg("pipeline")
    for prior in AIA_PRIORS:
        with pytest.raises(ValueError, match="bidirectional GRU"):
            pl.SamplerPipeline("cpu", prior, {}, {}, 2, L_=16000, ragged=True)
        with pytest.raises(ValueError, match="bidirectional GRU"):
            pl.SamplerPipeline("cpu", prior, {}, {}, 2, L_=16000, ragged=True, masked_prior=False)
        with pytest.raises(ValueError, match="L_"):
            pl.SamplerPipeline("cpu", prior, {}, {}, 2, T=20, ragged=True, masked_prior=True)


def test_descriptors_carry_the_tables_last_and_null():
    lib = pkg("_lib")
    so = lib.load()
    assert so.pdse_abi_version() == lib.ABI_VERSION == 9
    for kind in (lib.OP_ATTN, lib.OP_GRU, lib.OP_GNCOMB, lib.OP_AHAM):
        assert so.pdse_desc_size(kind) == C.sizeof(lib.DESC_TYPES[kind]), lib.DESC_TYPES[kind].__name__
    for typ, names in ((lib.AttnDesc, ("seqlen",)), (lib.GruDesc, ("seqlen",)),
                       (lib.GncombDesc, ("frames", "per_frame", "pad1_")), (lib.AhamDesc, ("frames", "per_frame", "pad1_"))):
        assert tuple(n for n, _ in typ._fields_[-len(names):]) == names
        assert all(not getattr(typ(), n) for n in names)        # a dense caller sets nothing
    # the fields in front of the tables sit where they sat: the new ones were appended
    assert lib.AttnDesc.seqlen.offset == 48 and lib.GruDesc.seqlen.offset == 80
    assert lib.GncombDesc.frames.offset == 104 and lib.AhamDesc.frames.offset == 80
    planfile = pkg("planfile")
    for typ in (lib.AttnDesc, lib.GruDesc, lib.GncombDesc, lib.AhamDesc):
        tab = getattr(typ, "seqlen", None) or typ.frames
        assert tab.offset in planfile.pointer_offsets(typ)


def test_launchers_refuse_tables_they_cannot_honour():
    """Validation happens before any launch, so it needs no device: a GRU along the inner axis has no per-item length, and
    the GroupNorm / AHAM tables need the size of a frame."""
    lib = pkg("_lib")
    buf = (C.c_float * 64)()
    ptr = C.addressof(buf)
    r = lib.GruDesc()
    r.whh, r.bhh, r.y, r.gx, r.seqlen = ptr, ptr, ptr, ptr, ptr
    r.B, r.T, r.F, r.H, r.axis = 1, 1, 1, 64, 0
    with pytest.raises(lib.PdseError, match="seqlen"):
        lib.launch(r)
    g = lib.GncombDesc()
    g.base = g.row = g.col = g.g_row = g.b_row = g.g_col = g.b_col = g.stats = g.out = g.frames = ptr
    g.plane, g.B, g.C = 4, 1, 1
    with pytest.raises(lib.PdseError, match="per_frame"):
        lib.launch(g)
    a = lib.AhamDesc()
    for i in range(4):
        a.x[i] = ptr
    a.w = a.means = a.out = a.frames = ptr
    a.plane, a.B, a.C = 4, 1, 1
    with pytest.raises(lib.PdseError, match="per_frame"):
        lib.launch(a)


def test_plan_builders_hand_the_table_to_the_instances_along_frames_only():
    """Recorded on a CPU context (descriptors only): with ``frames`` the column layers' attention and GRU, every GroupNorm
    update and both AHAM pools carry the table, the row layers' attention and GRU do not; without it nothing does."""
    import torch

    nets, synth, lib = pkg("nets"), pkg("synth"), pkg("_lib")
    B, T = 2, 9
    for cls, arch, n_aham in ((nets.AiaPlan, "aia_complex_trans_ri", 1), (nets.DualAiaPlan, "dual_aia_trans_merge_crm", 2)):
        sd = synth.make_state_dict(arch)
        for with_tab in (False, True):
            tab = torch.full((B,), T, dtype=torch.int32) if with_tab else None
            net = cls(nets.Ctx("cpu"), sd, B, T, frames=tab)
            net.descs = []
            net.build()
            ds = [d for d, _ in net.descs]
            attn = [d for d in ds if isinstance(d, lib.AttnDesc)]
            gru = [d for d in ds if isinstance(d, lib.GruDesc)]
            gn = [d for d in ds if isinstance(d, lib.GncombDesc)]
            ah = [d for d in ds if isinstance(d, lib.AhamDesc)]
            assert (len(attn), len(gru), len(gn), len(ah)) == (8, 8, 4, n_aham)
            want = tab.data_ptr() if with_tab else None
            for d in attn:                       # "ft" operands: the sequence is the innermost axis, F == T for the column layers
                along_frames = (d.T, d.F) == (net.FH, T)
                assert d.seqlen == (want if along_frames else None), (arch, with_tab)
            for d in gru:                        # axis 1: the sequence is the outer axis, T == T for the column layers
                along_frames = (d.T, d.F) == (T, net.FH)
                assert d.seqlen == (want if along_frames else None), (arch, with_tab)
            assert sum(d.seqlen is not None for d in attn) == sum(d.seqlen is not None for d in gru) == (4 if with_tab else 0)
            for d in gn + ah:
                assert d.frames == want and d.per_frame == (net.FH if with_tab else 0)


def test_main_parses_masked_prior(tmp_path, monkeypatch):
    main = pkg("main")
    monkeypatch.chdir(tmp_path)
    (tmp_path / "conf").mkdir()
    (tmp_path / "conf" / "dbaiat.yml").write_text("model:\n  name: aia_complex_trans_ri\n")
    base = ["--config", "dbaiat.yml", "--assets", str(tmp_path / "a"), "--generate", "--batch", "4"]
    args, config = main.parse_args_and_config(base + ["--masked-prior"])
    assert args.masked_prior is True and args.batch == 4 and config.model.name == "aia_complex_trans_ri"
    args, _ = main.parse_args_and_config(base)
    assert args.masked_prior is False
