"""The helper form of the register-weight 3x3 kernel (conv3x3_rw.hip: 64 -> 64 couts with GroupNorm + SiLU and 0 .. 3 skip
chunks run as blocks of 8 waves — four matrix waves, four helper waves that stage the input) against its 4-wave form (option
no_rw_helper, conv3x3_rw4.hip): torch.equal on the output AND on the int64 GroupNorm accumulators, in both libraries, plus the
per-element bound of tests/convcheck.py against the float64 reference.

Shapes: one tile per block (prologue and tail only); every border flag with a block boundary in the middle of a row; four tiles
per block under rw_quarter (ring wrap, steady state); uneven tile shares.  Variants: no skip chunk, residual (one identity
chunk), folded 1x1 skip on 64, 128 and 192 raw channels (192 as the concat of 64 + 128).  Each with and without statistics;
GroupNorm from a materialised table and — where the entry point takes them (conv2d_fused: no skip, residual) — from the
producer's accumulators.  The launches go through the launcher of tests/test_rw_gpu.py with option rw_small."""
import math

import pytest
import torch

import convcheck as CC
from diffsep_amd import _lib, ops, synth
from diffsep_amd.engine import Engine, pack_state_dict, param_table

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
DTS = {"bf16": torch.bfloat16, "f16": torch.float16}


def _set(name, v):
    for k in DTS:
        l = _lib.lib(k)
        _lib.check(l.diffsep_set_option(name, v), l)


@pytest.fixture(autouse=True, scope="module")
def _rw_small():
    _set(b"rw_small", 1)
    try:
        yield
    finally:
        _set(b"rw_small", 0)
        _set(b"no_rw_helper", 0)
        _set(b"rw_quarter", 0)


def rnd(tag, shape, scale=1.0):
    return torch.from_numpy(synth.synth_noise(tag, shape)) * scale


# (B, H, W, rw_quarter)
SHAPES = [(2, 32, 32, 0), (1, 40, 64, 0), (1, 256, 256, 1), (3, 64, 96, 0)]
# name, skip chunks, raw skip channels (first, second) | "res" | None
VARIANTS = [("nsk0", 0, None), ("res", 1, "res"), ("skip64", 1, (64, 0)), ("skip128", 2, (64, 64)), ("skip192", 3, (64, 128))]


@pytest.mark.parametrize("B,H,W,quarter", SHAPES)
@pytest.mark.parametrize("vname,nsk,extra", VARIANTS)
@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_helper_form_equals_four_wave_form(kind, vname, nsk, extra, B, H, W, quarter):
    dt = DTS[kind]
    tag = f"rwh{B}{H}{W}"
    # the input out of a producer launch, so that its accumulators exist: GroupNorm table from them, once
    xi = rnd(tag + ".xi", (B, H, W, 16)).to(DEV, dt)
    wi = ops.pack_conv_weight(rnd("rwh.wi", (64, 16, 3, 3), 1.0 / 12.0), dt).to(DEV)
    a, sa = ops.conv2d_fused(xi, wi, rnd("rwh.bi", (64,), 0.3).to(DEV), 64, 3, stats=True)
    gam, bet, groups = (1.0 + rnd("rwh.g", (64,), 0.2)).to(DEV), rnd("rwh.be", (64,), 0.1).to(DEV), 16
    sc, sh = ops.groupnorm_from_acc(sa, None, gam, bet, groups, H * W)
    w = rnd("rwh.w", (64, 64, 3, 3), 1.0 / 24.0)
    kc = ops.conv2d_chunk(3, dt)
    wp = ops.pack_conv_weight(w, dt, chunk=kc).to(DEV)
    bias, bb = rnd("rwh.bias", (64,), 0.1).to(DEV), rnd(tag + ".bb", (B, 64), 0.1).to(DEV)
    res = skip = skw = None
    if extra == "res":
        res = rnd(tag + ".r", (B, H, W, 64)).to(DEV, dt)
    elif extra is not None:
        s1, s2 = extra
        sw = rnd(f"rwh.sw{s1 + s2}", (64, s1 + s2, 1, 1), 1.0 / math.sqrt(s1 + s2))
        sxa = rnd(tag + f".sa{s1}", (B, H, W, s1)).to(DEV, dt)
        sxb = rnd(tag + f".sb{s2}", (B, H, W, s2)).to(DEV, dt) if s2 else None
        skip = (sxa, sxb, sw.reshape(64, -1).to(DEV, dt).contiguous())
        skw = (sxa, sxb, sw)
    osc = 0.70710678 if nsk else 1.0

    def run(stats, acc):
        if skip is not None:
            r = ops.conv3x3_regweight(a, wp, 64, gn=(sc, sh), bias=bias, bias_b=bb, skip=skip, out_scale=osc, stats=stats, w_chunk=kc)
        else:
            gn = dict(gn_acc=(sa, None, gam, bet, groups)) if acc else dict(gn=(sc, sh))
            r = ops.conv2d_fused(a, wp, bias, 64, 3, gn_act=1, bias_b=bb, res=res, out_scale=osc, stats=stats, w_chunk=kc, **gn)
        name = ops.last_conv_kernel(kind)
        assert name == f"conv3x3_rw_kernel<1,4,{nsk},2,2>", name
        return r if stats else (r, None)

    _set(b"rw_quarter", quarter)
    try:
        checked = False
        for stats in (True, False):
            for acc in ((False, True) if skip is None else (False,)):
                _set(b"no_rw_helper", 0)
                y, st = run(stats, acc)
                _set(b"no_rw_helper", 1)
                y4, st4 = run(stats, acc)
                what = f"{kind} {vname} {B}x{H}x{W} stats {stats} acc {acc}"
                assert bool(torch.isfinite(y.float()).all()) and float(y.float().abs().max()) > 0, what
                assert torch.equal(y, y4), what
                if stats:
                    assert torch.equal(st, st4) and int(st.abs().max()) > 0, what
                if not checked:  # (every other output of the case has the same bits)
                    packed = None if kind == "bf16" else ("pk_fold" if nsk == 0 else "pk")
                    CC.ConvCheck((a, None), (sc, sh, 1), w, dt, bias=bias, bb=bb, res=res, skip=skw, out_scale=osc, packed=packed)(y, what)
                    y0 = y
                    checked = True
                else:
                    assert torch.equal(y, y0), what
    finally:
        _set(b"no_rw_helper", 0)
        _set(b"rw_quarter", 0)


def test_kernel_names_of_an_evaluation_do_not_change():
    """one evaluation of the nf = 64 network in both forms: the same launch records (kernel name with its template arguments,
    shape, class), the helper-form instantiations among them, and the same bits out"""
    cfg = _lib.model_config(nf=64, num_sources=2, dtype=_lib.F16, spec_factor=0.33)
    sd = synth.synth_state_dict([(n, s) for n, s, _ in param_table(cfg)], 7)
    eng = Engine(cfg, pack_state_dict(cfg, sd))
    eng.set_option("rw_small", 1)
    mix = torch.from_numpy(synth.synth_batch(1, T=8000)[0]).to(DEV)
    mn, _, _ = ops.normalize_batch(mix)
    sde = dict(ndim=2, d_lambda=2.0, sigma_min=0.05, sigma_max=0.5)
    kw = dict(N=1, corrector_steps=1, snr=0.5, eps=0.03, denoise=True, seed=3)
    out, recs = [], []
    for v in (0, 1):
        eng.set_option("no_rw_helper", v)
        assert eng.get_option("no_rw_helper") == v
        eng.profile_begin()
        y, _ = eng.pc_sample(mn, sde, **kw)
        eng.profile_end()
        out.append(y)
        recs.append([(r["kernel"], r["cls"], r["B"], r["H"], r["W"], r["Cin"], r["Cout"], r["skip_cin"], r["has_res"])
                     for r in eng.profile_records()])
    eng.close()
    assert recs[0] == recs[1]
    names = {r[0] for r in recs[0]}
    assert any(n.startswith("conv3x3_rw_kernel<1,4,") and n.endswith(",2,2>") for n in names), names
    assert torch.equal(out[0], out[1])
