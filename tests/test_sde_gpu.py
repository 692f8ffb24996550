"""The kernels of csrc/sde.hip and their unit entries against the float64 references and per-element bounds of
tests/sdecheck.py (derivations, what each instrument sees and cannot see: that module's docstring; its CPU self-test:
tests/test_sdecheck_cpu.py).  Every [convcheck ...] line printed here is a worst err / bound; the gate is 1, and the values are
copied into sdecheck.MEASURED.

Cannot see: the Philox counter's high word (needs n > 2^34 values); the `lens` arguments of the three sampler updates, which
have no unit entry (the engine's batch-equals-single tests cover them); anything the host does not refuse is never launched with
arguments a kernel does not guard (a length above T, S > 4)."""
import ctypes

import numpy as np
import pytest
import torch

import sdecheck as C
from diffsep_amd import _lib, ops, synth

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
NAN = float("nan")


def D(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if a is not None else None


# ------------------------------------------------------------------------------------------------ noise
@pytest.mark.parametrize("seed", [0, 123, 2 ** 40 + 5, 2 ** 64 - 1])
def test_randn_matches_the_philox_reference(seed):
    w = 0.0
    for sid in (0, 1, 2 ** 32 + 1):
        for n in (1, 2, 3, 4, 5, 1023, 1024, 1025, 4099):
            out = ops.randn(n, seed, sid)
            w = max(w, C.check(out, C.randn_ref(n, seed, sid), f"randn n={n} seed={seed} sid={sid}"))
            if n == 4099:
                assert torch.equal(out, ops.randn(n, seed, sid))  # equal arguments: bit-equal output
    assert not torch.equal(ops.randn(4099, seed, 1), ops.randn(4099, seed, 2 ** 32 + 1))  # the stream id's high word counts
    print(f"[sdecheck randn seed={seed}] worst err / bound {w:.3f}")


def test_randn_of_nothing_launches_nothing():
    buf = torch.full((4,), NAN, device=DEV)
    _lib.call(_lib.lib(), "diffsep_randn", _lib._ptr(buf), 0, 5, 0, _lib._stream_ptr())
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())
    assert ops.randn(0, 5, 0).shape == (0,)  # (an empty tensor has no address; that is no error)


@pytest.mark.parametrize("S", [1, 3])
def test_randn_batch_layout_and_zero_tails(S):
    T, lens, seeds, sid = 9, [9, 1, 0, 6], [11, 2 ** 40 + 5, 3, 2 ** 64 - 1], 2 ** 32 + 1
    out = ops.randn_batch(4, S, T, seeds, lens, sid)
    C.check(out, C.randn_batch_ref(S, T, seeds, lens, sid), f"randn_batch S={S}")
    assert not bool(out[2].any())  # the zero-length utterance
    for b, n in enumerate(lens):
        assert not bool(out[b, :, n:].any())
        if n:
            assert torch.equal(out[b, :, :n].reshape(-1), ops.randn(S * n, seeds[b], sid)), b


# ------------------------------------------------------------------------------------------------ per-index kernels: the case table
T_TABLE = (1, 255, 256, 257, 1000)


@pytest.mark.parametrize("pmix", [False, True], ids=["MixSDE", "PriorMixSDE"])
@pytest.mark.parametrize("S", [1, 2, 3, 4])
def test_sampler_updates_case_table(S, pmix):
    sde = dict(C.PMIX if pmix else C.MIX, ndim=S)
    B, tt = 3, D(C.T_CASES)
    w = dict(prior=0.0, corrector=0.0, predictor=0.0)
    for T in T_TABLE:
        c = C.state_case(f"tab{S}{pmix}{T}", B, S, T, pmix)
        x, sc, z, y, sm = (D(c[k]) for k in ("x", "score", "z", "y", "smix"))
        tag = f"S={S} T={T} {'pmix' if pmix else 'mix'}"
        w["prior"] = max(w["prior"], C.check(ops.sde_prior(sde, y, z, sm), C.prior(sde, c["y"], c["z"], c["smix"]), "prior " + tag))
        # the prior's mean factor, seen on z = 0: 0.5 at S = 2 and under PriorMixSDE, 1 / S otherwise
        cf = np.float32(0.5) if (S == 2 or pmix) else np.float32(1.0) / np.float32(S)
        x0 = ops.sde_prior(sde, y, torch.zeros_like(z), sm)
        assert torch.equal(x0, D(cf * c["y"]).expand(B, S, T)), tag
        for variant in ((0,) if pmix else (0, 1)):
            xo, xm = ops.sde_corrector_update(sde, 0.5, x, tt, sc, z, sm, variant)
            rx, rm = C.corrector(sde, 0.5, c["x"], C.T_CASES, c["score"], c["z"], c["smix"], variant)
            w["corrector"] = max(w["corrector"], C.check(xo, rx, f"corrector {variant} x {tag}"), C.check(xm, rm, f"corrector {variant} mean {tag}"))
        for N in (1, 30):
            xo, xm = ops.sde_predictor_update(sde, N, x, tt, sc, z, sm)
            rx, rm = C.predictor(sde, N, c["x"], C.T_CASES, c["score"], c["z"], c["smix"])
            w["predictor"] = max(w["predictor"], C.check(xo, rx, f"predictor N={N} x {tag}"), C.check(xm, rm, f"predictor N={N} mean {tag}"))
            # probability flow: no noise, x == x_mean bit for bit, and z is not read (NaN would show)
            xo, xm = ops.sde_predictor_update(sde, N, x, tt, sc, torch.full_like(z, NAN), sm, probability_flow=True)
            rx, rm = C.predictor(sde, N, c["x"], C.T_CASES, c["score"], None, c["smix"], pflow=True)
            assert torch.equal(xo, xm), tag
            w["predictor"] = max(w["predictor"], C.check(xm, rm, f"probability flow N={N} {tag}"))
        if S == 1:  # the drift and the P part vanish: nothing depends on lambda (p and the drift multiply an exact zero)
            other = dict(sde, d_lambda=7.0)
            assert torch.equal(ops.sde_prior(sde, y, z, sm), ops.sde_prior(other, y, z, sm))
            for a, b in zip(ops.sde_corrector_update(sde, 0.5, x, tt, sc, z, sm), ops.sde_corrector_update(other, 0.5, x, tt, sc, z, sm)):
                assert torch.equal(a, b)
            for a, b in zip(ops.sde_predictor_update(sde, 30, x, tt, sc, z, sm), ops.sde_predictor_update(other, 30, x, tt, sc, z, sm)):
                assert torch.equal(a, b)
            assert not bool(ops.sde_coefficients(sde, x, tt, sm)[0].any())
    print(f"[sdecheck updates S={S} {'pmix' if pmix else 'mix'}] worst err / bound prior {w['prior']:.3f} corrector {w['corrector']:.3f} "
          f"predictor {w['predictor']:.3f}")


# ------------------------------------------------------------------------------------------------ the SDE object surface
@pytest.mark.parametrize("pmix", [False, True], ids=["MixSDE", "PriorMixSDE"])
@pytest.mark.parametrize("S", [1, 2, 3, 4])
def test_sde_surface(S, pmix):
    sde = dict(C.PMIX if pmix else C.MIX, ndim=S)
    B, tt = 3, D(C.T_CASES)
    w = {}

    def rec(k, r):
        w[k] = max(w.get(k, 0.0), r)
    for T in (1, 257):
        c = C.state_case(f"surf{S}{pmix}{T}", B, S, T, pmix)
        x, sc, sm = D(c["x"]), D(c["score"]), D(c["smix"])
        tag = f"S={S} T={T} {'pmix' if pmix else 'mix'}"
        dt = np.float32(1.0 / 30.0)
        for fs, gs in ((1.0, 1.0), (float(dt), float(np.sqrt(dt)))):
            drift, diff = ops.sde_coefficients(sde, x, tt, sm, fs, gs)
            rd, rg = C.sde_coefficients(sde, c["x"], C.T_CASES, c["smix"], fs, gs)
            rec("coeff", max(C.check(drift, rd, f"drift fs={fs:.3g} {tag}"), C.check(diff, rg, f"diffusion gs={gs:.3g} {tag}")))
        rec("mean", C.check(ops.sde_mean(sde, x, tt), C.sde_mean(sde, c["x"], C.T_CASES), "sde_mean " + tag))
        rec("std", C.check(ops.sde_std(sde, tt, S, T, sm), C.sde_std(sde, C.T_CASES, S, c["smix"], T=T), "sde_std " + tag))
        # mult_std on an arbitrary dense std (not one sde_std built), both layouts
        for shape in ((B, S, S), (B, S, S, T)):
            L = C.noise(f"surf.L{S}{T}{len(shape)}", shape)
            rec("mult_std", C.check(ops.sde_mult_std(D(L), x), C.sde_mult_std(L, c["x"]), f"mult_std {len(shape)}d {tag}"))
        f = C.noise(f"surf.f{S}{T}", (B, S, T), 0.3)
        for G in (np.abs(C.noise(f"surf.g{S}{T}", (B,), 0.5)), np.abs(C.noise(f"surf.G{S}{T}", (B, S, T), 0.5))):
            for pf in (False, True):
                rec("reverse", C.check(ops.sde_reverse_drift(D(f), D(G), sc, pf), C.sde_reverse_drift(f, G, c["score"], pf),
                                       f"reverse_drift G{G.ndim}d pflow={pf} {tag}"))
    print(f"[sdecheck surface S={S} {'pmix' if pmix else 'mix'}] worst err / bound " + " ".join(f"{k} {v:.3f}" for k, v in w.items()))


def test_wrappers_refuse_a_mismatched_sigma_mix():
    c = C.state_case("refuse", 3, 2, 5, True)
    x, sc, z, y, sm = (D(c[k]) for k in ("x", "score", "z", "y", "smix"))
    tt = D(C.T_CASES)
    text = "PriorMixSDE needs sigma_mix, MixSDE must not get one"
    for sde, s in ((C.MIX, sm), (C.PMIX, None)):
        for call in (lambda: ops.sde_prior(sde, y, z, s), lambda: ops.sde_corrector_update(sde, 0.5, x, tt, sc, z, s),
                     lambda: ops.sde_predictor_update(sde, 3, x, tt, sc, z, s), lambda: ops.sde_coefficients(sde, x, tt, s),
                     lambda: ops.sde_std(sde, tt, 2, 5, s)):
            with pytest.raises(_lib.DiffsepError, match=text):
                call()
    with pytest.raises(_lib.DiffsepError, match="corrector variant"):
        ops.sde_corrector_update(C.PMIX, 0.5, x, tt, sc, z, sm, variant=1)


def test_sigma_mix_windows_and_floor():
    m = C.sigma_mix_signals()
    floor = np.float32(0.5) * np.sqrt(np.float32(1e-4))
    w = 0.0
    for k in (1, 2, 3, 8, 509, 510, 2000):
        out = ops.sde_sigma_mix(D(m)[:, None], k)
        ref = C.sigma_mix(m, k)
        w = max(w, C.check(out, ref, f"sigma_mix avg_len={k}"))
        at = ref[0][1] == 0.5 * np.sqrt(C.SIGMA_FLOOR)
        assert bool((out[1].cpu().numpy()[at] == floor).all())  # the clamped outputs are the floor value itself
    print(f"[sdecheck sigma_mix] worst err / bound {w:.3f}")


# ------------------------------------------------------------------------------------------------ reductions
@pytest.mark.parametrize("T", [2, 1023, 1024, 1025, 3000])
def test_normalize_batch(T):
    mix = np.stack([C.noise(f"norm.a{T}", (1, T), 0.3) + np.float32(0.1), np.full((1, T), 0.1, np.float32),
                    np.float32(1000.0) + np.float32(1e-3) * C.noise(f"norm.c{T}", (1, T))]).astype(np.float32)
    out, mean, std = ops.normalize_batch(D(mix))
    r = C.normalize_batch(mix)
    w = [C.check(out, r["out"], f"normalize out T={T}"), C.check(mean.reshape(-1), r["mean"], f"normalize mean T={T}"),
         C.check(std.reshape(-1), r["std"], f"normalize std T={T}")]
    # a constant: output exactly 0, std exactly the floor
    assert not bool(out[1].any()) and float(std[1]) == float(np.float32(1e-5)) and float(mean[1]) == float(np.float32(0.1))
    print(f"[sdecheck normalize T={T}] worst err / bound out {w[0]:.3f} mean {w[1]:.3f} std {w[2]:.3f}")


@pytest.mark.parametrize("S", [1, 2, 3, 4])
def test_scale_output_and_gram(S):
    B, ws, wg = 2, 0.0, 0.0
    for T in (1, 2, 1023, 1024, 1025, 3000):
        mix, sep, est = C.noise(f"so.m{S}{T}", (B, 1, T)), C.noise(f"so.s{S}{T}", (B, S, T), 0.7), C.noise(f"so.e{S}{T}", (B, S, T))
        ws = max(ws, C.check(ops.scale_output(D(mix), D(sep)), C.scale_output(mix, sep), f"scale_output S={S} T={T}"))
        zero = ops.scale_output(D(mix), torch.zeros((B, S, T), device=DEV))
        assert not bool(zero.any()) and bool(torch.isfinite(zero).all())
        wg = max(wg, C.check(ops.gram(D(sep), D(est)), C.gram(sep, est), f"gram S={S} T={T}"))
    print(f"[sdecheck reductions S={S}] worst err / bound scale_output {ws:.3f} gram {wg:.3f}")


@pytest.mark.parametrize("n", [1, 1025])
@pytest.mark.parametrize("B", [1, 3])
def test_langevin_update(B, n):
    x, g, z = C.noise(f"lv.x{B}{n}", (B, 1, n), 0.5), C.noise(f"lv.g{B}{n}", (B, 1, n), 2.0), C.noise(f"lv.z{B}{n}", (B, 1, n))
    xo, xm = ops.sde_langevin_update(0.5, D(x), D(g), D(z))
    rx, rm, step = C.langevin(0.5, x, g, z)
    w = max(C.check(xo, rx, f"langevin x B={B} n={n}"), C.check(xm, rm, f"langevin mean B={B} n={n}"))
    if B == 3:  # one step size for the batch: utterance 2's score moves utterance 0's output as the reference says
        g2 = g.copy()
        g2[2] *= np.float32(3.0)
        xo2, xm2 = ops.sde_langevin_update(0.5, D(x), D(g2), D(z))
        rx2, rm2, step2 = C.langevin(0.5, x, g2, z)
        assert step2 < 0.9 * step and (np.abs(rm2[0][0] - rm[0][0]) > rm[1][0] + rm2[1][0]).any()
        w = max(w, C.check(xo2, rx2, f"langevin x, other score, B={B} n={n}"), C.check(xm2, rm2, f"langevin mean, other score, B={B} n={n}"))
        assert not torch.equal(xm2[0], xm[0])
    print(f"[sdecheck langevin B={B} n={n}] worst err / bound {w:.3f}")


# ------------------------------------------------------------------------------------------------ time embedding
@pytest.mark.parametrize("nf", [8, 16, 24, 32, 64])
def test_time_embedding_elementwise(nf):
    shapes = [("all_modules.0.W", (nf,)), ("all_modules.1.weight", (4 * nf, 2 * nf)), ("all_modules.1.bias", (4 * nf,)),
              ("all_modules.2.weight", (4 * nf, 4 * nf)), ("all_modules.2.bias", (4 * nf,))]
    sd = synth.synth_state_dict(shapes, 7)
    p = [sd[k] for k, _ in shapes]
    t = np.array([1.0, 0.53, 0.2, 0.03, 1e-3], np.float32)
    out = ops.time_embedding(D(t), *(D(v) for v in p))
    w = C.check(out, C.time_embedding(t, *p), f"time embedding nf={nf}")
    print(f"[sdecheck time embedding nf={nf}] worst err / bound {w:.3f}")


# ------------------------------------------------------------------------------------------------ dtype conversion
def _convert_vector(kind):
    """float32 values: random, exact ties of round-to-nearest-even in both directions, +-0, +-inf, NaN, the largest finite fp32
    (overflows to inf), and, for half, its subnormal range"""
    v = []
    r = np.abs(C.noise("cv.t." + kind, (16,))).astype(np.float32) + np.float32(0.5)
    bits = r.view(np.uint32).copy()
    if kind == "bf16":
        lo, half, keep = np.uint32(0xFFFF), np.uint32(0x8000), 16
    else:
        lo, half, keep = np.uint32(0x1FFF), np.uint32(0x1000), 13
    base = bits & ~lo
    even = base & ~(np.uint32(1) << np.uint32(keep))  # kept lsb 0: the tie rounds down
    odd = base | (np.uint32(1) << np.uint32(keep))    # kept lsb 1: the tie rounds up
    ties = np.concatenate([even | half, odd | half]).view(np.float32)
    v += [ties, -ties]
    v.append(np.array([0.0, -0.0, np.inf, -np.inf, np.nan, np.finfo(np.float32).max, -np.finfo(np.float32).max], np.float32))
    if kind == "f16":
        v.append((np.arange(-40, 41, dtype=np.float32) * np.float32(2.0 ** -25) * np.float32(0.5)).astype(np.float32))  # ties and values below 2^-14
        v.append(np.array([2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, 65504.0, 65519.9, 65520.0, 1e-8], np.float32))
    v.append(C.noise("cv." + kind, (4096,), 3.0))  # (the edge values come first: every n >= 255 holds all of them)
    out = np.concatenate(v).astype(np.float32)
    assert out.size - 4096 <= 255
    return out


def _same_bits(a, b, what):
    a, b = a.cpu(), b.cpu()
    nan = torch.isnan(b.float())
    assert torch.equal(torch.isnan(a.float()), nan), what + ": a NaN did not stay a NaN"
    ib = torch.int32 if a.dtype == torch.float32 else torch.int16
    assert torch.equal(a.view(ib)[~nan], b.view(ib)[~nan]), what


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_convert_is_bit_exact_in_both_builds(kind):
    half = torch.bfloat16 if kind == "bf16" else torch.float16
    base = _convert_vector(kind)
    for n in (1, 255, 256, 257, 8192 * 256 + 3):  # the last takes the grid-stride loop round once
        src = torch.from_numpy(np.resize(base, n))
        d = src.to(DEV)
        h = ops.convert(d, half, kind)
        _same_bits(h, src.to(half), f"{kind} fp32 -> 16 n={n}")
        _same_bits(ops.convert(h, torch.float32, kind), src.to(half).float(), f"{kind} 16 -> fp32 n={n}")
        _same_bits(ops.convert(d, torch.float32, kind), src, f"{kind} fp32 -> fp32 n={n}")
        _same_bits(ops.convert(h, half, kind), src.to(half), f"{kind} 16 -> 16 n={n}")
    head = torch.from_numpy(base[:255])
    assert int(torch.isinf(head.to(half).float()).sum()) > int(torch.isinf(head).sum()) and bool(torch.isnan(head.to(half).float()).any())
    assert bool((head.to(half).float() != head)[:64].all())  # the ties do round


def test_convert_refuses_unknown_dtype_codes():
    a, b = torch.zeros(8, device=DEV), torch.full((8,), NAN, device=DEV)
    for kind in ("bf16", "f16"):
        for sd, dd in ((2, 0), (0, 2), (3, 1), (-1, 0)):
            with pytest.raises(_lib.DiffsepError, match="convert: dtype"):
                _lib.call(_lib.lib(kind), "diffsep_convert", _lib._ptr(a), _lib._ptr(b), 8, sd, dd, _lib._stream_ptr())
    torch.cuda.synchronize()
    assert bool(torch.isnan(b).all())  # refused on the host: nothing was launched


# ------------------------------------------------------------------------------------------------ the wide Dense_0 projection
@pytest.mark.parametrize("K,outs,B", C.dense_cases(), ids=lambda v: str(v).replace(" ", ""))
def test_dense_projection(K, outs, B):
    # exact integers: every product and partial sum is exact in fp32 in any order
    x, ws, bs = C.int_case(f"dp{K}{outs}{B}", B, K, outs)
    y = ops.dense_projection(D(x), [D(w) for w in ws], [D(b) for b in bs], silu_in=False)
    ref, _ = C.dense_projection(x, ws, bs, silu_in=False)
    assert torch.equal(y.cpu().double(), torch.from_numpy(ref)), (K, outs, B)
    # per-element bound on random data through the SiLU
    x, ws, bs = C.rand_case(f"dp{K}{outs}{B}", B, K, outs)
    y = ops.dense_projection(D(x), [D(w) for w in ws], [D(b) for b in bs], silu_in=True)
    w = C.check(y, C.dense_projection(x, ws, bs, silu_in=True), f"dense projection K={K} O={outs} B={B}")
    if (outs, B) == ((65,), 17):  # bias = null
        y = ops.dense_projection(D(x), [D(v) for v in ws], None, silu_in=True)
        w = max(w, C.check(y, C.dense_projection(x, ws, None, silu_in=True), f"dense projection, no bias, K={K}"))
    print(f"[sdecheck dense K={K} O={outs} B={B}] worst err / bound {w:.3f}")


def test_dense_projection_refuses_k_on_the_host():
    # K = 2048 would ask the generic kernel for 128 KiB of dynamic LDS, above what a launch may request without opting in
    for K, text in ((2048, "at most 1024"), (1028, "at most 1024"), (6, "multiple of 4"), (0, "multiple of 4")):
        x, w = torch.zeros((2, max(K, 1)), device=DEV), torch.zeros((3, max(K, 1)), device=DEV)
        y, ws = torch.full((2, 3), NAN, device=DEV), torch.empty(3 * max(K, 1), device=DEV)
        oc = (ctypes.c_int32 * 1)(3)
        with pytest.raises(_lib.DiffsepError, match=text):
            _lib.call(_lib.lib(), "diffsep_dense_projection", _lib._ptr(x), _lib._ptr(w), None, oc, 1, _lib._ptr(y), 2, K, 1, _lib._ptr(ws),
                      ws.numel() * 4, _lib._stream_ptr())
        torch.cuda.synchronize()
        assert bool(torch.isnan(y).all())
