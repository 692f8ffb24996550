"""The references and inputs of tests/test_attn_fused_gpu.py are fit for purpose (no GPU needed).  For every case:
  * ref_exact, fed M = Wk^T Wq and b' = Wk^T b_q folded from NIN parameters, is the CPU oracle's AttnBlockpp (1e-5: fp32 oracle);
  * the residual is at most 1/8 of the attention branch, and the mean effective number of keys lies between 2 and L / 2;
  * the mirror run in float32 stays within 0.25 E_round of the mirror in float64: the reference alone is inside gate 2;
  * on every ragged L, a mask that is off by one key in either direction moves the mirror's y by more than 5 x gate 2, and one
    padded row added to the channel sums breaks gate 3 in float16.
So the GPU gates fail for a kernel that is wrong in those ways."""
import functools

import pytest
import torch

import attn_fused_ref as R
import diffsep_oracle as O

torch.set_grad_enabled(False)
CASES = [(L, dt) for dt in R.DTYPES for L in R.L_ALL]
IDS = [f"L{L}-{R.dt_id(dt)}" for L, dt in CASES]
RAGGED = [(L, dt) for dt in R.DTYPES for L in R.L_RAGGED]
RAGGED_IDS = [f"L{L}-{R.dt_id(dt)}" for L, dt in RAGGED]
GATE2 = 0.5


@functools.lru_cache(maxsize=None)
def refs(L, dt):
    op = R.unit_case(L, dt)
    ex, mir = R.attn_ref(op), R.attn_ref(op, mirror=True)
    return op, ex, mir, R.rel_rms(mir.y, ex.v)


@pytest.mark.parametrize("L,dt", CASES, ids=IDS)
def test_exact_reference_is_the_oracle_block(L, dt):
    H, W = 4, L // 4
    bc = R.block_case(H, W, dt)
    ref = O._attn_block(O.to_torch(bc.sd), "", bc.x).permute(0, 2, 3, 1).reshape(R.BATCH, L, R.C)
    assert R.rel_rms(R.attn_ref(bc.exact).v, ref) <= 1e-5


@pytest.mark.parametrize("L,dt", CASES, ids=IDS)
def test_inputs_let_the_attention_branch_carry_the_output(L, dt):
    op, ex, _, _ = refs(L, dt)
    assert R.rms(op.x) <= R.rms(ex.branch) / 8.0
    assert 2.0 <= R.effective_keys(ex.P) <= L / 2.0


@pytest.mark.parametrize("H,W", R.BLOCK_HW)
@pytest.mark.parametrize("dt", R.DTYPES, ids=R.dt_id)
def test_block_inputs_let_the_attention_branch_carry_the_output(H, W, dt):
    bc = R.block_case(H, W, dt)
    ex = R.attn_ref(bc.exact)
    assert R.rms(bc.x) <= R.rms(ex.branch) / 8.0
    assert 2.0 <= R.effective_keys(ex.P) <= H * W / 2.0


@pytest.mark.parametrize("L,dt", CASES, ids=IDS)
def test_float32_mirror_is_inside_gate_2(L, dt):
    op, _, mir, E = refs(L, dt)
    m32 = R.attn_ref(op, mirror=True, cdt=torch.float32)
    r = R.rel_rms(m32.y, mir.y) / E
    print(f"\n[attn_fused ref {R.dt_id(dt)} L={L}] E_round {E:.2e}  f32 mirror {r:.3f}")
    assert r <= 0.25


@pytest.mark.parametrize("L,dt", RAGGED, ids=RAGGED_IDS)
def test_mask_off_by_one_key_breaks_gate_2(L, dt):
    op, _, mir, E = refs(L, dt)
    dropped = R.attn_ref(op, mirror=True, keys=L - 1)  # key L - 1 masked
    added = R.attn_ref(op, mirror=True, keys=L + 1)    # key L (a zero h row: V = b_v) not masked
    assert R.rel_rms(dropped.y, mir.y) > 5.0 * GATE2 * E
    assert R.rel_rms(added.y[:, :L], mir.y) > 5.0 * GATE2 * E


@pytest.mark.parametrize("L", R.L_RAGGED)
def test_counted_padded_row_breaks_gate_3_in_float16(L):
    op, _, mir, E = refs(L, R.HF)
    pad = R.attn_ref(op, mirror=True, rows=L + 1).v[:, L]  # what the kernel computes for the first row past L
    sum_abs, sum_sq = R.gate_terms(mir)
    assert torch.equal(R.attn_ref(op, mirror=True, rows=L + 1).s1, mir.s1)  # (the reference itself counts L rows)
    assert bool((pad.abs() > 0.5 * E * sum_abs).any()) and bool((pad ** 2 > E * sum_sq).any())
    # not a marginal break: most (sample, channel) sums leave the gate
    assert float((pad.abs() > 0.5 * E * sum_abs).double().mean()) > 0.5
