"""CPU: (1) the statement of one block-kernel launch in tests/helpers/bglu_refs.py against encoder / decoder stages assembled
here from torch.nn's Conv2d / ConvTranspose2d / ConstantPad2d / BatchNorm2d (eval) / PReLU in double, loaded with the same
synthetic state dict - both stage kinds, the stage-1 composition, the chained conv1 of the next stage, and the rounding
route of the statement with the rounding replaced by the identity; (2) every case of tests/helpers/bglu_cases.py - the
descriptors tests/test_gpu_bglu_ops.py launches - replayed on tests/emu.py (run_bglu, run_planes) under the checks the GPU
file applies, which pins the builder, the packers and the case table without a GPU, together with the f16x2 window of every
np = 2 case; (3) the builder against the product: all 15 stages of a small nets.EpsNetPlan at np 1 / 2 / 3, scalar fields, tap
tables and qexp equal, packed weights byte for byte; (4) the case table holds every geometry kind for every form."""
import ctypes as C

import numpy as np
import pytest
import torch
from torch import nn

import emu
from conftest import pkg
from helpers import bglu_cases as G
from helpers import bglu_refs as R

TOL = dict(atol=1e-12, rtol=1e-12)
F64 = torch.float64


# ------------------------------------------------------------------ the reference against torch
class TorchBlock(nn.Module):
    """BiConvGLU / BiConvTransGLU behind its conv1, as the network assembles it."""

    def __init__(self, cin, cout, kw, transposed):
        super().__init__()
        conv = nn.ConvTranspose2d if transposed else nn.Conv2d
        self.conv1 = conv(cin, 32, (1, 1))
        self.l, self.r = conv(32, 32, (2, kw), stride=(1, 2)), conv(32, 32, (2, kw), stride=(1, 2))
        self.l_conv, self.r_conv, self.conv2 = conv(32, 32, (1, 1)), conv(32, 32, (1, 1)), conv(32, cout, (1, 1))

    def block(self, h):
        left, right = self.l(h), self.r(h)
        return self.conv2(left * torch.sigmoid(self.r_conv(right)) + right * torch.sigmoid(self.l_conv(left)))


def _load(mod, sd, prefix):
    own = {k: sd[prefix + "." + k].double() for k in mod.state_dict() if prefix + "." + k in sd}
    mod.load_state_dict(own, strict=False)
    return mod.double().eval()


def _bn_prelu(sd, bn, prelu):
    m = nn.Sequential(nn.BatchNorm2d(64), nn.PReLU()).double().eval()
    m[0].load_state_dict({k: sd["%s.%s" % (bn, k)].double() for k in ("weight", "bias", "running_mean", "running_var")}, strict=False)
    m[1].weight.data[:] = sd[prelu].double()
    return m


def _case(form, **kw):
    return G._c("host_%s" % form, form=form, **kw)


@pytest.mark.parametrize("form,B,T,Fin,params", [("enc", 2, 3, 11, "hostile"), ("enc", 1, 1, 8, "nominal"), ("enc5", 2, 4, 9, "hostile")])
def test_ref_matches_torch_encoder_stage(form, B, T, Fin, params):
    c = _case(form, B=B, T=T, Fin=Fin, params=params)
    kind, k = G.STAGE[form]
    sd, temb = G.make_sd(c), torch.from_numpy(G.make_temb(c, B))
    p = G.natural(sd, kind, k, 0, temb.numpy())
    h = torch.randn(B, 32, T, Fin, generator=torch.Generator().manual_seed(T), dtype=F64)
    blk = _load(TorchBlock(64, 64, 3, False), sd, "en.conv%d" % k)
    post = _bn_prelu(sd, "en.en%d.0" % k, "en.en%d.1.weight" % k)
    pad = nn.ConstantPad2d((0, 0, 1, 0), 0.0)
    with torch.no_grad():
        want = post(blk.block(pad(h)))
    got = R.encoder(p, F64, h=h)
    torch.testing.assert_close(got["Y"], want, **TOL)
    if form == "enc":                               # the three chained conv1, each behind its own time projection
        nxt = _load(TorchBlock(64, 64, 3, False), sd, "en.conv%d" % (k + 1))
        tp = nn.Linear(512, 64).double()
        tp.load_state_dict({k_: sd["en.tp%d.%s" % (k + 1, k_)].double() for k_ in ("weight", "bias")})
        with torch.no_grad():
            torch.testing.assert_close(got["Z"][0], nxt.conv1(want + tp(temb)[:, :, None, None]), **TOL)
            for i, de in enumerate(G.DECS):
                q = "%s.de%d.0" % (de, k)
                d1 = _load(TorchBlock(128, 64, 3, True), sd, q)
                t128 = temb @ sd[q + ".tp.weight"].double().T + sd[q + ".tp.bias"].double()
                # the decoder's conv1 over cat(x, skip) + t: the skip half with the whole bias, the other half without one
                z = torch.zeros(B, 64, T, want.shape[-1], dtype=F64)
                full = d1.conv1(torch.cat([z, want], 1) + t128[:, :, None, None])
                torch.testing.assert_close(got["Z"][1 + i], full, **TOL)


@pytest.mark.parametrize("B,T,Fin,params", [(2, 3, 13, "hostile"), (1, 1, 12, "nominal")])
def test_ref_matches_torch_stage1(B, T, Fin, params):
    """Preprocess, the causal pad, the time projection, conv1, the block, BatchNorm, PReLU as the network runs them."""
    c = _case("enc1", B=B, T=T, Fin=Fin, params=params)
    sd, temb = G.make_sd(c), torch.from_numpy(G.make_temb(c, B))
    p = G.natural(sd, "en", 1, 0, temb.numpy())
    g = torch.Generator().manual_seed(5)
    x0, x1 = (torch.randn(B, 2, T, Fin, generator=g, dtype=F64) for _ in range(2))
    pre = nn.Conv2d(4, 2, (1, 1)).double()
    pre.load_state_dict({k_: sd["preprocess.conv." + k_].double() for k_ in ("weight", "bias")})
    blk = _load(TorchBlock(2, 64, 5, False), sd, "en.conv1")
    post = _bn_prelu(sd, "en.en1.0", "en.en1.1.weight")
    pad = nn.ConstantPad2d((0, 0, 1, 0), 0.0)
    tp = temb @ sd["en.tp1.weight"].double().T + sd["en.tp1.bias"].double()
    with torch.no_grad():
        want = post(blk.block(blk.conv1(pad(pre(torch.cat([x0, x1], 1))) + tp[:, :, None, None])))
    torch.testing.assert_close(R.encoder(p, F64, x0=x0, x1=x1)["Y"], want, **TOL)
    # the route the rounding statement takes (composed weights on the inputs, the rest as biases), rounding nothing
    same = R.encoder(p, F64, x0=x0, x1=x1, q=lambda v: v)
    torch.testing.assert_close(same["Y"], want, atol=1e-11, rtol=1e-11)


@pytest.mark.parametrize("form,B,T,Fin,params", [("dec", 2, 3, 5, "hostile"), ("dec", 1, 1, 4, "nominal"), ("dec1", 2, 3, 6, "hostile")])
def test_ref_matches_torch_decoder_stage(form, B, T, Fin, params):
    c = _case(form, B=B, T=T, Fin=Fin, params=params, di=1)
    kind, k = G.STAGE[form]
    sd = G.make_sd(c)
    p = G.natural(sd, kind, k, 1, G.make_temb(c, B))
    de = G.DECS[1]
    g = torch.Generator().manual_seed(9)
    h = torch.randn(B, 32, T, Fin, generator=g, dtype=F64)
    blk = _load(TorchBlock(128, 64 if k > 1 else 1, 3 if k > 1 else 5, True), sd, "%s.de%d.0" % (de, k))
    with torch.no_grad():
        y = blk.block(h)[:, :, :-1]                                         # Chomp_T(1)
    if k == 1:
        torch.testing.assert_close(R.decoder(p, h, F64)["out"], y[:, 0], **TOL)
        return
    with torch.no_grad():
        want = _bn_prelu(sd, "%s.de%d.2" % (de, k), "%s.de%d.3.weight" % (de, k))(y)
    add = torch.randn(B, 32, T, want.shape[-1], generator=g, dtype=F64)
    got = R.decoder(p, h, F64, add=add)
    torch.testing.assert_close(got["Y"], want, **TOL)
    nxt = nn.ConvTranspose2d(128, 32, (1, 1), bias=False).double()
    nxt.weight.data[:] = sd["%s.de%d.0.conv1.weight" % (de, k - 1)].double()
    with torch.no_grad():
        z = nxt(torch.cat([want, torch.zeros_like(want)], 1)) + add
    torch.testing.assert_close(got["Z"][0], z, **TOL)
    # the rounding route with the identity for a rounding is the same statement (the folded operands unfold exactly enough)
    torch.testing.assert_close(R.decoder(p, h, F64, add=add, q=lambda v: v)["Z"][0], z, atol=1e-10, rtol=1e-10)


def test_ref_stage5_conv1_matches_torch():
    g = torch.Generator().manual_seed(2)
    xs = [torch.randn(2, 64, 3, 4, generator=g, dtype=F64) for _ in range(2)]
    m = nn.ConvTranspose2d(128, 32, (1, 1)).double()
    bias = torch.randn(2, 32, generator=g, dtype=F64)
    with torch.no_grad():
        want = m(torch.cat(xs, 1)) - m.bias[None, :, None, None] + bias[:, :, None, None]
    torch.testing.assert_close(R.conv1_cat(xs, [m.weight[:, :, 0, 0].T.detach()], [bias])[0], want, **TOL)


def test_ref_bf16_rounding_points():
    """rnd moves the result by about what a handful of roundings of 2^-9 cost - neither nothing nor another operation."""
    from conftest import rel_l2

    for name in ("encnp1_tiles_B2_T9_F40", "decnp1_small_B3_T1_F4"):
        b = G.build(G.find(name), "cpu")
        plain, rnd = b.ref(F64), b.ref(F64, True)
        e = rel_l2(rnd["Z"][0], plain["Z"][0])
        assert 2.0 ** -12 < e < 2.0 ** -5, e


# ------------------------------------------------------------------ the case table on the emulator
def _window(b):
    """np = 2: every tensor the launch splits into fp16 planes inside the f16x2 window, |value| * 2^PDSE_F16_ACT_EXP < 65504
    with the issue's factor two to spare: the inputs, L, R, G, Y and the chained tile's result."""
    if b.np != 2:
        return
    r = b.ref(F64)
    ts = [r["L"], r["R"], r["G"]] + ([r["Y"]] if "Y" in r else []) + list(r.get("Z", []))[:1]
    ts += [b.h_in] if b.h_in is not None else list(b.x)
    for t in ts:
        assert float(t.abs().max()) < 4094.0 / 2, b.case["id"]


@pytest.mark.parametrize("case", G.ALL, ids=G.by_id(G.ALL))
def test_emulator_bglu(case):
    b = G.build(case, "cpu")
    _window(b)
    emu.run_bglu(b.desc, emu.Mem(G.tensors(b)))
    G.verify(b)


@pytest.mark.parametrize("npl", [3, 2, 1])
def test_emulator_planes_conv(npl):
    """Every planes_conv case.  emu.run_planes writes whole items (hp_split: zero margins where the kernel leaves the pattern),
    so the margin check alone is off in the replay; values, own elements and sources are held as on the GPU."""
    for case in [c for c in G.PC_CASES if c["np"] == npl]:
        b = G.build_pc(case, "cpu")
        emu.run_planes(b.desc, emu.Mem(G.tensors(b)))
        G.verify_pc(b, strict=False)


def test_case_table_reaches_what_it_names():
    """For each of the five forms and each plane count: one partial tile at T = 1; several tiles, neither P a multiple of 32 nor
    the tiles of 8; more rounds than workgroups with uneven trip counts and a partial last round; B = 1.  Across the table:
    odd and even bin counts into the parity-split forms, Fout1 = Fout - 1 in every decoder case, constant and per-item biases,
    nx_row0 on and off, both decoders' channels of the last stage, the weight groups' qexp at three values or more, ten apart."""
    L = pkg("_lib")
    for npl in (3, 2, 1):
        for form in G.FORMS:
            cs = [c for c in G.CASES[npl] if c["form"] == form]
            have = set().union(*(G.kinds(c) for c in cs))
            assert have == {"small", "tiles", "rounds", "B1"}, (form, npl, have)
            assert any(G.launch_geom(c)["rounds"] == 3 and G.launch_geom(c)["gx"] == 2 for c in cs)
            if form in ("enc", "enc5"):
                assert {c["Fin"] & 1 for c in cs} == {0, 1}
            if form in ("dec", "dec1"):
                assert all(G.geom(form, c["Fin"])["Fout1"] == G.geom(form, c["Fin"])["Fout"] - 1 for c in cs)
            if form == "dec1":
                assert {c["di"] for c in cs} == {0, 1}
            built = [G.build(c, "cpu") for c in cs if c["B"] <= 3]
            assert {bool(b.desc.bias_sb) for b in built} == {False, True}, form
            if form in ("enc1", "enc"):
                assert {b.desc.nx_row0 for b in built} == {0, 1} and {bool(b.desc.nx_bias_sb[0]) for b in built} == {False, True}
                assert all(b.desc.nx_par == 1 and b.desc.nx_items == b.B + 1 for b in built)
            if npl == 2:
                for b in built:
                    if b.case["ws"] is not None:
                        q = tuple(b.desc.qexp)
                        live = q[:2] + ((q[2],) if form != "dec1" else ()) + ((q[3],) if b.desc.nx_n else ())
                        assert len(set(live)) >= min(3, len(live)) and max(live) - min(live) >= 10, (b.case["id"], q)
    hostile = G.make_sd(G.find("encnp3_small_B3_T1_F19"))
    s = hostile["en.en2.0.weight"].numpy()
    assert int((s == 0).sum()) == 2 and (s < 0).any() and (s > 0).any() and float(hostile["en.en2.0.running_var"].min()) < 2.1e-3
    assert float(hostile["en.en2.1.weight"][0]) in G.SLOPES
    assert {float(G.make_sd(c)[k][0]) for c in G.ALL for k in G.make_sd(c) if k.endswith((".1.weight", ".3.weight"))} == set(G.SLOPES)
    lb = hostile["en.conv2.l_conv.bias"].numpy()
    assert int((lb == 30).sum()) >= 6 and int((lb == -30).sum()) >= 6
    assert isinstance(G.build(G.find("encnp3_small_B3_T1_F19"), "cpu").desc, L.BgluDesc) and G.WGS == 256


# ------------------------------------------------------------------ the builder against nets.EpsNetPlan
def _scalars(d):
    def scal(v):
        if isinstance(v, C.Structure):
            return {n: scal(getattr(v, n)) for n, t in v._fields_ if t is not C.c_void_p}
        if isinstance(v, C.Array):
            return None if v._type_ is C.c_void_p else [scal(e) for e in v]
        return v

    return scal(d)


@pytest.mark.parametrize("npl", [1, 2, 3])
def test_builder_matches_eps_net_plan(weights, npl):
    """All 15 block launches of a plan: scalar fields (everything but pointers), tap tables and qexp equal; packed weights and
    the constant operands byte for byte; the time-conditioned biases against what the plan's time launch leaves (fp32 folding
    against this file's float64: 1e-5 of the largest)."""
    nets, L = pkg("nets"), pkg("_lib")
    sd = weights("DiffUNet1")
    B, T = 2, 3
    ctx = nets.Ctx("cpu")
    net = nets.EpsNetPlan(ctx, sd, B, T, time_cond=True, nsteps=1, planes=npl)
    net.tsteps[0] = torch.tensor([3.0, 11.5])
    net.build_time()
    net.build_step(0)
    emu.run(net.descs, ctx.all_tensors(), net.time_index, net.time_index + 1)
    temb = net.temb[0].numpy().astype(np.float64)
    mem = emu.Mem(ctx.all_tensors())
    descs = [d for d, _ in net.descs if isinstance(d, L.BgluDesc)]
    stages = [("en", k, 0) for k in range(1, 6)] + [("de", k, di) for di in (0, 1) for k in (5, 4, 3, 2, 1)]
    assert len(descs) == 15
    for d, (kind, k, di) in zip(descs, stages):
        Fin = net.ENC_F[k - 1] if kind == "en" else net.ENC_F[k]
        b = G.build_stage(sd, kind, k, di, B, T, Fin, npl, "cpu", temb)
        assert _scalars(b.desc) == _scalars(d), (kind, k, di)
        own = emu.Mem(G.tensors(b))
        for key, v in b.fields.items():
            if not isinstance(v, np.ndarray):
                continue
            dt = np.int16 if v.dtype == np.uint16 else np.float32
            n = v.size
            assert np.asarray(mem.arr(getattr(d, key), n, dt)).tobytes() == np.asarray(own.arr(getattr(b.desc, key), n, dt)).tobytes(), (kind, k, di, key)
        if kind == "en" and k < 5:
            ptrs = [(d.nx_bias[i], b.desc.nx_bias[i]) for i in range(3)]
            if k == 1:
                ptrs += [(getattr(d, f), getattr(b.desc, f)) for f in ("bias0", "bias1", "bias0_t0", "bias1_t0")]
            for theirs, mine in ptrs:
                for item in range(B):
                    a, w = mem.arr(theirs + 4 * item * G.SBB, 32), own.arr(mine + 4 * item * G.SBB, 32)
                    assert np.abs(a - w).max() <= 1e-5 * np.abs(w).max(), (kind, k)
