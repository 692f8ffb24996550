"""The walk of tests/netcheck.py on the device: every tensor one eager score evaluation stores (engine option "trace"), each against
the float64 reference of the operation that produced it, fed with the device's own stored inputs.  Gate: err / bound <= 1 per
element with the unit instruments' bounds, unchanged; nothing is fitted to device output.  H = 256 rows, W = 64 frames
(eng.bucket_length(64)), where tests/golden/conv_routes.json recorded the routes; B >= 2 with a different t per row in every case (a
batch-stride fault is invisible at B = 1 or with equal rows).  synth_state_dict(..., 7) and noise inputs of scale 0.3 keep every
layer's stored input inside the instruments' domain |x sc| + |sh| <= 32 (ConvCheck / GnCheck assert it).

One score evaluation per (engine, options, B); the walk is parametrized by segment and row level so that each test stays at a few
seconds of float64 reference on the CPU.  Both closure assertions (every record claimed by one step, every step finds its record) hold
when a Walk is constructed, i.e. in every test below.

Cases: nf = 16 fp32 with S = 2 and S = 3; nf = 64 at B = 2 in bfloat16, half, split-fp32 and fp32 (whole walk); nf = 64 bfloat16
at B = 4: the steps whose kernel differs from the B = 2 run (the tile-count flips); nf = 64 bfloat16 with no_attn_fused: the
attention blocks (fused by default: 128 channels at 16 rows); nf = 128 bfloat16 at B = 2: the cat(128, 128) -> 128 blocks of the 256-
and 128-row levels under the default options, no_sw, and no_sw + no_split256, and the attention blocks (256 channels: the unfused chain
whatever the options, so no_attn_fused must change nothing there).
"""
import functools

import pytest
import torch

import netcheck as NC
import stftcheck as SC
from diffsep_amd import _lib, synth
from diffsep_amd.engine import Engine, pack_state_dict, param_table

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
W_FRAMES, SEED, IN_SCALE = 64, 7, 0.3
TIMES = (0.03, 0.8, 0.3, 0.1)
LEVELS = [256 >> i for i in range(7)]
GROUPS = ["front"] + [("down", h) for h in LEVELS] + [("mid", LEVELS[-1])] + [("up", h) for h in reversed(LEVELS)] + ["back"]
GROUP_IDS = [g if isinstance(g, str) else f"{g[0]}{g[1]}" for g in GROUPS]
DTYPES = {"bf16": _lib.BF16, "f16": _lib.F16, "split": _lib.F32_SPLIT, "f32": _lib.F32}
WORST = {}


@functools.lru_cache(None)
def engine(nf, dtype, S=2):
    cfg = _lib.model_config(nf=nf, num_sources=S, dtype=DTYPES[dtype])
    sd = synth.synth_state_dict([(n, s) for n, s, _ in param_table(cfg)], SEED)
    return Engine(cfg, pack_state_dict(cfg, sd)), sd


def evaluate(nf, dtype, S, B, options):
    eng, sd = engine(nf, dtype, S)
    T = eng.bucket_length(W_FRAMES)
    assert eng.padded_frames(T) == W_FRAMES
    xt, mix = SC.signal(f"nw.gpu{B}.{S}", B, S, T, IN_SCALE)
    t = torch.tensor(TIMES[:B], dtype=torch.float32)
    prov = NC.EngineProvider(eng, sd, NC.cfg_dict(nf, num_sources=S), xt.float(), t, mix.float(), options=options)
    return NC.Walk(prov)  # (both closure assertions)


@functools.lru_cache(None)
def walk(nf, dtype, S=2, B=2, options=()):
    return evaluate(nf, dtype, S, B, options)


@functools.lru_cache(1)
def walk128(options, B=2):
    """nf = 128: one evaluation kept at a time (its snapshot of the arena is the largest)"""
    return evaluate(128, "bf16", 2, B, options)


def run(w, tag, select):
    ratios = w.run(select=select)
    NC.report(tag, ratios)
    for k, v in ratios.items():
        WORST[(tag.split(" /")[0], k)] = max(WORST.get((tag.split(" /")[0], k), 0.0), v)
    assert all(v <= 1.0 for v in ratios.values())
    return ratios


def in_group(g):
    return lambda s: s.group == g


@pytest.mark.parametrize("g", GROUPS, ids=GROUP_IDS)
@pytest.mark.parametrize("S", [2, 3])
def test_walk_nf16_fp32(S, g):
    w = walk(16, "f32", S)
    assert set(w.groups()) == set(GROUPS)
    run(w, f"nf16 f32 S={S} / {g}", in_group(g))
    assert w.ran > 0


@pytest.mark.parametrize("g", GROUPS, ids=GROUP_IDS)
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_walk_nf64(dtype, g):
    w = walk(64, dtype)
    assert set(w.groups()) == set(GROUPS)
    assert {r["B"] for r in w.p.records} == {2}
    run(w, f"nf64 {dtype} / {g}", in_group(g))
    assert w.ran > 0


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_nf64_attention_is_the_fused_kernel(dtype):
    w = walk(64, dtype)
    fused = [s for s in w.steps if s.kind == "attn_fused"]  # (the three blocks of the 16-row level; the middle one has L = 4: unfused)
    assert len(fused) == 3 and all(s.kernel.startswith("attn_fused_kernel<") and s.group[1] == 16 for s in fused), [s.kernel for s in fused]
    assert any(s.kind == "attention" and s.group == ("mid", 4) for s in w.steps)


def test_walk_nf64_bf16_unfused_attention():
    w = walk(64, "bf16", options=("no_attn_fused",))
    attn = [s for s in w.steps if "attention" in s.name]
    assert attn and not any(s.kind == "attn_fused" for s in attn) and {"attention", "gemm", "gn_apply", "table"} <= {s.kind for s in attn}
    run(w, "nf64 bf16 no_attn_fused / attention", lambda s: "attention" in s.name)


def test_walk_nf64_bf16_tile_count_flips_at_batch_4():
    w2, w4 = walk(64, "bf16"), walk(64, "bf16", B=4)
    k2 = {s.key: s.kernel for s in w2.steps}
    assert set(k2) == {s.key for s in w4.steps}
    flips = [s for s in w4.steps if s.kernel != k2[s.key]]
    print(f"[netcheck nf64 bf16 B=4] {len(flips)} steps change kernel against B = 2: "
          f"{sorted({(k2[s.key].split('<')[0], s.kernel.split('<')[0]) for s in flips})}")
    assert flips, "no launch changes its kernel between B = 2 and B = 4: the case checks nothing"
    assert {r["B"] for r in w4.p.records} == {4}
    run(w4, "nf64 bf16 B=4 / flips", lambda s: s in flips)


CAT128 = "(cat 256->128)"
OPTION_SETS = {"default": (), "no_sw": ("no_sw",), "no_sw+no_split256": ("no_sw", "no_split256")}


def cat_steps(w, rows):
    return [s for s in w.steps if CAT128 in s.name and s.group == ("up", rows)]


@pytest.mark.parametrize("rows", [256, 128])
@pytest.mark.parametrize("opts", list(OPTION_SETS))
def test_walk_nf128_cat_blocks(opts, rows):
    w = walk128(OPTION_SETS[opts])
    steps = cat_steps(w, rows)
    assert len({s.mod for s in steps}) == (3 if rows == 256 else 2)  # (the first block of the 128-row level is cat(256, 128))
    roles = {o.rec["role"] for s in steps for o in s.outs}
    kernels = {s.name.split(") ", 1)[1]: s.kernel for s in steps}
    print(f"[netcheck nf128 {opts} {rows} rows] roles {sorted(roles)}; kernels {sorted(set(kernels.values()))}")
    conv0 = [s.kernel for s in steps if "Conv_0" in s.name]
    # (the routes differ at 256 rows; at B = 2 the 128-row level has too few tiles for any of them and takes the generic tile under
    # all three option sets on a 256-CU device: walked all the same, its kernels printed above)
    if opts == "default" and rows == 256:  # the streamed-weight kernel: Conv_1 with the whole 256-channel skip folded
        assert "outp" not in roles
        assert all(s.kernel.startswith("conv3x3_sw_kernel<") for s in steps if "folded Conv_2" in s.name)
        assert any(k.startswith("conv3x3_sw_kernel<") for k in conv0)
    elif opts == "no_sw" and rows == 256:  # the two register-weight launches of each convolution (one 4 x 32 tile per CU at B = 2)
        assert {"h1p", "h1", "outp", "out"} <= roles
        assert all(k.startswith("conv3x3_rw_kernel<") for k in conv0), conv0
    elif opts == "no_sw+no_split256":     # the generic tile on the concat
        assert "h1p" not in roles and "outp" not in roles
        assert all(k.startswith("conv_mfma_kernel<") for k in conv0), conv0
    run(w, f"nf128 bf16 {opts} / cat blocks {rows}", lambda s: s in steps)


@pytest.mark.parametrize("opts", [(), ("no_attn_fused",)], ids=["default", "no_attn_fused"])
def test_walk_nf128_attention(opts):
    w = walk128(opts)
    attn = [s for s in w.steps if "attention" in s.name]
    assert len({s.mod for s in attn}) == 4 and not any(s.kind == "attn_fused" for s in attn)  # (256 channels: never the fused kernel)
    run(w, "nf128 bf16 / attention", lambda s: "attention" in s.name)


def test_zz_report_worst_ratios():
    """the figures of this run, per engine and step kind (copied into netcheck.MEASURED and DESIGN.md as records)"""
    for (tag, kind), v in sorted(WORST.items()):
        print(f"[netcheck worst] {tag}: {kind}: {v:.3f}")
