"""The fused attention kernel (csrc/attn_fused.hip) against plain float64 references (tests/attn_fused_ref.py), at every
compile-time tile count LT = 1, 2, 4, 8, whole and ragged L = H * W, in both storage types, with its output statistics.

Inputs make the attention branch carry the output (x small, GroupNorm scale large: the residual is under 1/8 of the branch), keep
the softmax between uniform and one-hot, and give b_o a non-zero mean; tests/test_attn_fused_ref_cpu.py proves those properties
and that each gate below fails for a mask that is off by one key or a padded row that is counted.

E_round = rel_rms(ref_mirror.y, ref_exact.v) is the size of the kernel's designed storage rounding, computed per case from the
references alone.  Gates per case (B = 3, one table per sample):
  1. rel_rms(y, ref_exact.v) <= 1.5 E_round;
  2. rel_rms(y, ref_mirror.y) <= 0.5 E_round (the sharp one: the references' own fp32 noise is the "f32" column below);
  3. channel sums of the output (stats=True) per sample and channel: |sum v - mirror| <= 0.5 E_round sum |v|,
     |sum v^2 - mirror| <= E_round sum v^2, over the rows r < L only;
  4. a sentinel sample behind the B samples of out= and of the statistics buffer keeps its bits;
  5. sample b of the batch equals its own B = 1 launch (torch.equal), output and statistics;
  6. L = 48, 192: the gn_acc= form equals the gn=groupnorm_from_acc(...) form bit for bit, and passes gate 1 with the float64
     GroupNorm table;
  7. L = 8, 24, 272 and C = 64 are refused and the output buffer is untouched.
Block level (ops.attnblock_forward, NIN parameters, 16 x 4 and 16 x 12): gate 1 against ref_exact with M = Wk^T Wq folded in
float64, and the fused kernel is what ran.

Per case: E_round, the float32 mirror against the float64 mirror (CPU), and the kernel's measured ratios to E_round
(MI355X; "exact" is gate 1, limit 1.5, "mirror" is gate 2, limit 0.5):

    storage   L   LT  E_round   f32    exact  mirror
    bfloat16   16  1  4.34e-03  0.009    -      -
    bfloat16   32  1  3.97e-03  0.039    -      -
    bfloat16   48  2  3.79e-03  0.052    -      -
    bfloat16   64  2  4.27e-03  0.047    -      -
    bfloat16   80  4  3.92e-03  0.010    -      -
    bfloat16  112  4  3.68e-03  0.043    -      -
    bfloat16  128  4  3.73e-03  0.045    -      -
    bfloat16  144  8  3.68e-03  0.024    -      -
    bfloat16  192  8  3.63e-03  0.025    -      -
    bfloat16  240  8  3.27e-03  0.024    -      -
    bfloat16  256  8  3.45e-03  0.034    -      -
    float16    16  1  5.47e-04  0.141    -      -
    float16    32  1  5.03e-04  0.125    -      -
    float16    48  2  5.11e-04  0.125    -      -
    float16    64  2  5.20e-04  0.131    -      -
    float16    80  4  4.91e-04  0.098    -      -
    float16   112  4  4.52e-04  0.145    -      -
    float16   128  4  4.67e-04  0.177    -      -
    float16   144  8  4.57e-04  0.117    -      -
    float16   192  8  4.54e-04  0.145    -      -
    float16   240  8  4.20e-04  0.163    -      -
    float16   256  8  4.35e-04  0.143    -      -

("-": not measured yet; each test prints its figures, run with -s)
"""
import functools

import pytest
import torch

import attn_fused_ref as R
from diffsep_amd import _lib, ops

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
C, B = R.C, R.BATCH
CASES = [(L, dt) for dt in R.DTYPES for L in R.L_ALL]
IDS = [f"L{L}-{R.dt_id(dt)}" for L, dt in CASES]
SENTINEL, STAT_SENTINEL = 7.0, 0x5A5A5A5A5A5A


def kind_of(dt):
    return "f16" if dt == R.HF else "bf16"


def lt_of(L):
    return next(lt for lt, ls in R.L_BY_LT.items() if L in ls)


def bits(t):
    return t.view(torch.int16)


def packed(op):
    """the device operands of ops.attn_fused after x: fragment-major weights (already in the storage type: exact), fp32 biases"""
    dt = op.x.dtype
    ws = [ops.pack_frag_weight(w.float().reshape(C, C, 1, 1), dt).to(DEV) for w in (op.M, op.Wv, op.Wo)]
    return ws + [b.float().to(DEV) for b in (op.bq, op.bv, op.bo)]


def launch(op, x, table, nb):
    """one launch on nb samples into buffers of nb + 1: (y buffer, statistics buffer) on the CPU and the kernel's name"""
    out = torch.full((nb + 1, op.L, C), SENTINEL, dtype=x.dtype, device=DEV)
    st = torch.zeros((nb + 1, C, 2), dtype=torch.int64, device=DEV)
    st[nb] = STAT_SENTINEL
    y, s = ops.attn_fused(x, *packed(op), gn=table, stats=st, out=out)
    assert y is out and s is st
    name = ops.last_conv_kernel(kind_of(x.dtype))
    torch.cuda.synchronize()
    return out.cpu(), st.cpu(), name


@functools.lru_cache(maxsize=None)
def refs(L, dt):
    op = R.unit_case(L, dt)
    ex, mir = R.attn_ref(op), R.attn_ref(op, mirror=True)
    return op, ex, mir, R.rel_rms(mir.y, ex.v)


@functools.lru_cache(maxsize=None)
def run(L, dt):
    op = refs(L, dt)[0]
    return launch(op, op.x.to(DEV), (op.scale.to(DEV), op.shift.to(DEV)), B)


@pytest.mark.parametrize("L,dt", CASES, ids=IDS)
def test_output_within_the_designed_rounding_of_both_references(L, dt):
    _, ex, mir, E = refs(L, dt)
    out, _, name = run(L, dt)
    assert name == f"attn_fused_kernel<{lt_of(L)}>", name
    y = out[:B]
    assert bool(torch.isfinite(y.float()).all())
    r_exact, r_mirror = R.rel_rms(y, ex.v) / E, R.rel_rms(y, mir.y) / E
    print(f"\n[attn_fused {R.dt_id(dt)} L={L} LT={lt_of(L)}] E_round {E:.2e}  exact {r_exact:.3f}  mirror {r_mirror:.3f}")
    assert r_exact <= 1.5
    assert r_mirror <= 0.5


@pytest.mark.parametrize("L,dt", CASES, ids=IDS)
def test_statistics_count_the_rows_of_the_sample_only(L, dt):
    _, _, mir, E = refs(L, dt)
    _, st, _ = run(L, dt)
    s = ops.stats_to_float(st[:B])
    sum_abs, sum_sq = R.gate_terms(mir)
    d1, d2 = (s[..., 0] - mir.s1).abs() / (E * sum_abs), (s[..., 1] - mir.s2).abs() / (E * sum_sq)
    print(f"\n[attn_fused stats {R.dt_id(dt)} L={L}] worst sum {float(d1.max()):.3f} (limit 0.5), sum of squares {float(d2.max()):.3f} (limit 1)")
    assert bool((d1 <= 0.5).all())
    assert bool((d2 <= 1.0).all())


@pytest.mark.parametrize("L,dt", CASES, ids=IDS)
def test_nothing_is_written_behind_the_batch(L, dt):
    out, st, _ = run(L, dt)
    assert torch.equal(bits(out[B]), bits(torch.full((L, C), SENTINEL, dtype=dt)))
    assert torch.equal(st[B], torch.full((C, 2), STAT_SENTINEL, dtype=torch.int64))
    assert not bool((bits(out[:B]) == bits(torch.full((1,), SENTINEL, dtype=dt))).all(-1).any())  # every row was written


@pytest.mark.parametrize("L,dt", CASES, ids=IDS)
def test_a_sample_does_not_depend_on_its_batch(L, dt):
    op = refs(L, dt)[0]
    out, st, _ = run(L, dt)
    for b in range(B):
        o1, s1, _ = launch(op, op.x[b:b + 1].to(DEV), (op.scale[b:b + 1].to(DEV), op.shift[b:b + 1].to(DEV)), 1)
        assert torch.equal(bits(o1[0]), bits(out[b]))
        assert torch.equal(s1[0], st[b])


@pytest.mark.parametrize("L,dt", [(L, dt) for dt in R.DTYPES for L in R.L_ACC],
                         ids=[f"L{L}-{R.dt_id(dt)}" for dt in R.DTYPES for L in R.L_ACC])
def test_table_from_accumulators_at_ragged_and_large_L(L, dt):
    op = R.acc_case(L, dt)
    ex, mir = R.attn_ref(op), R.attn_ref(op, mirror=True)
    E = R.rel_rms(mir.y, ex.v)
    # accumulators as a producing convolution would leave them: fixed-point sums of the stored tensor
    xd = op.x.double()
    acc = torch.stack([(xd.sum(1) * ops.STAT_SUM_SCALE).round(), ((xd * xd).sum(1) * ops.STAT_SQ_SCALE).round()], -1)
    acc = acc.to(torch.int64).contiguous().to(DEV)
    g, be, x = op.gamma.to(DEV), op.beta.to(DEV), op.x.to(DEV)
    y_acc, st_acc = ops.attn_fused(x, *packed(op), gn_acc=(acc, g, be, R.GROUPS), stats=True)
    table = ops.groupnorm_from_acc(acc, None, g, be, R.GROUPS, L)
    y_tab, st_tab = ops.attn_fused(x, *packed(op), gn=table, stats=True)
    assert torch.equal(bits(y_acc), bits(y_tab)) and torch.equal(st_acc, st_tab)
    r = R.rel_rms(y_acc, ex.v) / E
    print(f"\n[attn_fused gn_acc {R.dt_id(dt)} L={L}] E_round {E:.2e}  exact {r:.3f}  mirror {R.rel_rms(y_acc, mir.y) / E:.3f}")
    assert r <= 1.5


@pytest.mark.parametrize("dt", R.DTYPES, ids=R.dt_id)
@pytest.mark.parametrize("L,Cc", [(8, C), (24, C), (272, C), (64, 64)])
def test_unsupported_shapes_are_refused_and_nothing_is_written(L, Cc, dt):
    op = R.unit_case(64, dt)
    x = torch.zeros((B, L, Cc), dtype=dt, device=DEV)
    out = torch.full((B + 1, L, Cc), SENTINEL, dtype=dt, device=DEV)
    with pytest.raises(_lib.DiffsepError):
        ops.attn_fused(x, *packed(op), gn=(op.scale.to(DEV), op.shift.to(DEV)), out=out)
    torch.cuda.synchronize()
    assert torch.equal(bits(out.cpu()), bits(torch.full((B + 1, L, Cc), SENTINEL, dtype=dt)))


@pytest.mark.parametrize("dt", R.DTYPES, ids=R.dt_id)
@pytest.mark.parametrize("H,W", R.BLOCK_HW)
def test_block_through_the_engine_code(H, W, dt):
    bc = R.block_case(H, W, dt)
    ex, mir = R.attn_ref(bc.exact), R.attn_ref(bc.mirror, mirror=True)
    E = R.rel_rms(mir.y, ex.v)
    assert R.rms(bc.x) <= R.rms(ex.branch) / 8.0
    y = ops.attnblock_forward(bc.params, ops.to_nhwc(bc.x).to(DEV, dt))
    assert ops.last_conv_kernel(kind_of(dt)) == f"attn_fused_kernel<{lt_of(H * W)}>"
    r = R.rel_rms(y.reshape(B, H * W, C), ex.v) / E
    print(f"\n[attn_fused block {R.dt_id(dt)} {H}x{W}] E_round {E:.2e}  exact {r:.3f}")
    assert r <= 1.5
