"""The STFT / iSTFT front end (csrc/stft.hip) on the device: every route, asserted by the kernel name the launch recorded
(ops.last_conv_kernel), against the float64 references and per-element bounds of tests/stftcheck.py.

Routes (forward | inverse):
  fused-bf16 / fused-f16  stft_fused_kernel<S+1> | istft_fused_kernel<NS,EM> of the two builds
  f32 / f32-split         stft_frame_kernel + DFT GEMM + stft_pack_kernel<f32> | istft_unpack_kernel<float> + GEMM + istft_ola_kernel,
                          the GEMM with fp32 or bf16x3 products
  thin-bf16 / thin-f16    the same three launches on 16-bit tensors (stft_pack_kernel<bf16|f16>, istft_unpack_kernel<bf16_t>), taken
                          under the process option no_stft_fused, which is set and restored around the launch
Every case asserts the name, then max |got - ref| / bound < 1 (printed), then the older tests' relative RMS at its old tolerance.
The zero-tail code of the inverse kernels is unreachable at n_fft = 510, hop = 128 (tests/test_stftcheck_cpu.py) and is not
exercised here."""
import contextlib
import functools
import os

import pytest
import torch

import stftcheck as sc
from stftcheck import BF, HF, F32
from diffsep_amd import _lib, ops

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
KIND = {BF: "bf16", HF: "f16", F32: "bf16"}     # the library a tensor of this type goes to
TNAME = {BF: "bf16", HF: "f16", F32: "f32"}


class Route:
    def __init__(self, rid, dt, split, thin, bound):
        self.id, self.dt, self.split, self.thin, self.bound = rid, dt, split, thin, bound
        self.values = dt if dt != F32 else BF   # the 16-bit type an inverse input is rounded to

    def __repr__(self):
        return self.id


ROUTES = [Route("fused-bf16", BF, False, False, "fused"), Route("fused-f16", HF, False, False, "fused"),
          Route("f32", F32, False, False, "f32"), Route("f32-split", F32, True, False, "split"),
          Route("thin-bf16", BF, False, True, "f32"), Route("thin-f16", HF, False, True, "f32")]
FUSED = ROUTES[:2]
ROUTE_IDS = [r.id for r in ROUTES]
# the older tests' relative-RMS gates (test_round5_gpu.py, test_kernels_gpu.py).  The split GEMM has none of its own: it forms the
# fused kernels' products and takes their gate (forward: the half-precision build's, the tighter)
FWD_RMS = {"fused-bf16": 5e-3, "fused-f16": 6e-4, "f32": 2e-5, "f32-split": 6e-4, "thin-bf16": 5e-3, "thin-f16": 6e-4}
INV_RMS = {"fused-bf16": 3e-5, "fused-f16": 3e-5, "f32": 2e-5, "f32-split": 3e-5, "thin-bf16": 2e-5, "thin-f16": 2e-5}


def fwd_name(r, S):
    return f"stft_fused_kernel<{S + 1}>" if r.bound == "fused" else f"stft_pack_kernel<{TNAME[r.dt]}>"


def inv_name(r, S, exponent):
    em = 0 if sc.f32(exponent) == 0.5 else (1 if sc.f32(exponent) == 1.0 else 2)
    return f"istft_fused_kernel<{2 if S == 2 else 1},{em}>" if r.bound == "fused" else "istft_ola_kernel"


@functools.lru_cache(None)
def _can_toggle(kind):
    """no_stft_fused can be set and cleared again in library `kind` (and is not this process's default already)"""
    if os.environ.get("DIFFSEP_NO_STFT_FUSED", "0") not in ("", "0"):
        return False
    L = _lib.lib(kind)
    return L.diffsep_set_option(b"no_stft_fused", 1) == 0 and L.diffsep_set_option(b"no_stft_fused", 0) == 0


@contextlib.contextmanager
def routed(r):
    """the process option of the three-launch 16-bit routes, restored whatever happens"""
    if not r.thin:
        yield
        return
    kind = KIND[r.dt]
    if not _can_toggle(kind):
        pytest.skip("the process option no_stft_fused cannot be set and restored here")
    L = _lib.lib(kind)
    _lib.check(L.diffsep_set_option(b"no_stft_fused", 1), L)
    try:
        yield
    finally:
        _lib.check(L.diffsep_set_option(b"no_stft_fused", 0), L)


def run_fwd(r, xt, mix, W, exponent=0.5, factor=0.33, shift=False):
    with routed(r):
        y = ops.stft_pack(xt.to(DEV), mix.to(DEV), W, 8, exponent=exponent, factor=factor, shift=shift, dtype=r.dt, split=r.split)
        name = ops.last_conv_kernel(KIND[r.dt])
    assert name == fwd_name(r, xt.shape[1]), (name, fwd_name(r, xt.shape[1]))
    return y.cpu()


def run_inv(r, x, S, T, exponent=0.5, factor=0.33, lay=(None, None, None), check_name=True):
    """x: a CPU tensor in the route's 16-bit type; the fp32 routes get the same values as float32.  The output is written into a
    buffer with one extra batch entry of markers, which must survive."""
    B = x.shape[0]
    xd = (x.float() if r.dt == F32 else x).to(DEV)
    out = torch.full((B + 1, S, T), 12345.0, dtype=torch.float32, device=DEV)
    ow, ob, td = (None if t is None else t.to(DEV) for t in lay)
    with routed(r):
        ops.istft_unpack(xd, S, T, exponent=exponent, factor=factor, split=r.split, ow=ow, ob=ob, tdiv=td, out=out)
        name = ops.last_conv_kernel(KIND[r.dt])
    if check_name:
        assert name == inv_name(r, S, exponent), (name, inv_name(r, S, exponent))
    out = out.cpu()
    assert bool((out[B] == 12345.0).all()), "the launch wrote past its batch"
    return out[:B]


# ------------------------------------------------------------------------------------------------ forward
FWD = dict(sc.fwd_cases())


@functools.lru_cache(None)
def fwd_ref(cid):
    c = FWD[cid]
    xt, mix = sc.fwd_input(cid, c)
    return xt, mix, sc.stft_ref(xt, mix, sc.FWD_W[c["T"]], c["exponent"], c["factor"], c["shift"])


def check_fwd(tag, r, y, ref):
    NC, F_ = ref["S"] + 1, ref["F"]
    assert y.dtype == r.dt and tuple(y.shape) == tuple(ref["y"].shape)
    assert bool((y[:, :, F_:, :2 * NC] == (-1.0 if ref["shift"] else 0.0)).all()), "padded frames"
    assert bool((y[..., 2 * NC:] == 0).all()), "padded channels"
    ratio = sc.worst_ratio(y, ref["y"], sc.stft_bound(ref, r.bound, r.dt))
    rms = sc.rel_rms(y, ref["y"])
    print(f"\n[stft {r.id} {tag}] err / bound {ratio:.3f}, rel rms {rms:.2e} (limit {FWD_RMS[r.id]:g})")
    assert ratio < 1.0
    assert rms < FWD_RMS[r.id]
    return ratio


@pytest.mark.parametrize("r", ROUTES, ids=ROUTE_IDS)
@pytest.mark.parametrize("cid", list(FWD))
def test_stft_against_float64_reference(cid, r):
    c = FWD[cid]
    xt, mix, ref = fwd_ref(cid)
    y = run_fwd(r, xt, mix, sc.FWD_W[c["T"]], c["exponent"], c["factor"], c["shift"])
    check_fwd(cid, r, y, ref)


@pytest.mark.parametrize("shift", [False, True])
@pytest.mark.parametrize("r", ROUTES, ids=ROUTE_IDS)
def test_stft_batch_entries_are_independent(r, shift):
    # entry 1 of 3 is silent: its real frames are exactly 0 (-1 shifted) whatever its neighbours hold; on the fused route (one block
    # per 32 frames of ONE entry, samples staged in LDS) entries 0 and 2 equal their own B = 1 launches bit for bit
    T, S, W = 3714, 2, 64
    xt, mix = sc.signal("stft.batch", 3, S, T)
    xt[1], mix[1] = 0.0, 0.0
    y = run_fwd(r, xt, mix, W, shift=shift)
    assert bool((y[1, :, :, :2 * (S + 1)] == (-1.0 if shift else 0.0)).all())
    check_fwd(f"B3 shift{int(shift)}", r, y, sc.stft_ref(xt, mix, W, shift=shift))
    if r.bound == "fused":
        for b in (0, 2):
            assert torch.equal(run_fwd(r, xt[b:b + 1], mix[b:b + 1], W, shift=shift)[0], y[b]), b


@pytest.mark.parametrize("r", [ROUTES[0], ROUTES[1], ROUTES[2]], ids=ROUTE_IDS[:3])
def test_stft_impulse_across_the_tile_edge(r):
    # an impulse reaches exactly the frames whose taps 1 .. 509 cover it, on both sides of frame 32, the first of the second tile
    xt, mix = sc.impulse_input()
    ref = sc.stft_ref(xt, mix, 64)
    y = run_fwd(r, xt, mix, 64)
    for b, n0 in enumerate(sc.IMPULSES):
        energy = (y[b, :, :, 0].double() ** 2 + y[b, :, :, 3].double() ** 2).sum(0)
        hit = [f for f in range(64) if energy[f] > 0]
        assert hit == sc.impulse_frames(n0), (n0, hit, sc.impulse_frames(n0))
    assert not bool(y[..., [1, 2, 4, 5, 6, 7]].any()), "the silent channels stay silent"
    check_fwd("impulse", r, y, ref)


# ------------------------------------------------------------------------------------------------ inverse
INV = dict(sc.inv_cases())


@functools.lru_cache(None)
def inv_ref(cid, dt):
    c = INV[cid]
    x, lay = sc.inv_input(cid, c, dt)
    return x, lay, sc.istft_ref(x, c["S"], c["T"], c["exponent"], c["factor"], *lay)


def check_inv(tag, r, out, ref, show_bound=False):
    bound = sc.istft_bound(ref, r.bound)
    ratio, rms = sc.worst_ratio(out, ref["out"], bound), sc.rel_rms(out, ref["out"])
    extra = f", mean bound / mean |out| {float(bound.mean() / ref['out'].abs().mean()):.2e}" if show_bound else ""
    print(f"\n[istft {r.id} {tag}] err / bound {ratio:.3f}, rel rms {rms:.2e} (limit {INV_RMS[r.id]:g}){extra}")
    assert bool(torch.isfinite(out).all())
    assert ratio < 1.0
    assert rms < INV_RMS[r.id]


# (pixels of +-300 are a half-precision input: the large case runs on the routes that read half precision)
INV_PAIRS = [(cid, r) for cid in INV for r in ROUTES if INV[cid]["kind"] != "large" or r.values == HF]


@pytest.mark.parametrize("cid,r", INV_PAIRS, ids=[f"{cid}-{r.id}" for cid, r in INV_PAIRS])
def test_istft_against_float64_reference(cid, r):
    c = INV[cid]
    x, lay, ref = inv_ref(cid, HF if c["kind"] == "large" else r.values)
    out = run_inv(r, x, c["S"], c["T"], c["exponent"], c["factor"], lay)
    check_inv(cid, r, out, ref, show_bound=c["kind"] == "large")


@pytest.mark.parametrize("f", sc.ONEHOT_F)
@pytest.mark.parametrize("r", [ROUTES[0], ROUTES[1], ROUTES[2]], ids=ROUTE_IDS[:3])
def test_istft_one_hot_pixels(r, f):
    # ONE non-zero pixel per batch entry: the output is exactly 0 outside the frame's support — in the other source, which shares
    # the block at NS = 2, in every other segment and overlap-add copy — and inside the bound on it
    T, S = sc.ONEHOT_T, 2
    x, probes = sc.onehot_input(f, r.values)
    ref = sc.istft_ref(x, S, T)
    out = run_inv(r, x, S, T)
    lo, hi = sc.support(f, T)
    for j, (k, s, imag) in enumerate(probes):
        assert not bool(out[j, 1 - s].any()), (j, "the other source")
        assert not bool(out[j, s, :lo].any()) and not bool(out[j, s, hi:].any()), (j, "outside the support")
        if imag and k in (0, 255):
            assert not bool(out[j].any()), (j, "the imaginary part of DC / Nyquist is ignored")
        elif hi > lo:                                   # (frame F - 1 starts at sample 128 (F - 1) - 255 = T: it reaches no sample)
            assert bool(out[j, s, lo:hi].any())
    ratio = sc.worst_ratio(out, ref["out"], sc.istft_bound(ref, r.bound))
    print(f"\n[istft {r.id} one-hot frame {f}] err / bound {ratio:.3f}")
    assert ratio < 1.0


@pytest.mark.parametrize("with_layer", [False, True])
@pytest.mark.parametrize("r", ROUTES, ids=ROUTE_IDS)
def test_istft_ignores_padded_frames_and_channels(r, with_layer):
    # NaN in frames [F, W), 1e3 in the channels nobody reads ([2S, ld) without the output layer, [ow_cin, ld) with it)
    T, S, ld = 3713, 2, 16
    c = dict(B=2, S=S, T=T, ld=ld, layer=with_layer, kind="noise")
    x, lay = sc.inv_input("istft.ignored", c, r.values)
    clean = run_inv(r, x, S, T, lay=lay)
    dirty = x.clone()
    dirty[:, :, sc.n_frames(T):] = float("nan")
    dirty[..., (2 * (S + 1) if with_layer else 2 * S):] = 1e3
    assert torch.equal(run_inv(r, dirty, S, T, lay=lay), clean)


@pytest.mark.parametrize("r", [ROUTES[0], ROUTES[1], ROUTES[2], ROUTES[4]], ids=[ROUTE_IDS[i] for i in (0, 1, 2, 4)])
def test_istft_refuses_an_output_layer_narrower_than_its_sources(r):
    # ow_cin < 2 S: the fused kernel and istft_unpack_kernel would disagree on the missing weights; both routes refuse
    T, S = 300, 2
    x, _ = sc.inv_input("istft.refuse", dict(B=2, S=S, T=T, ld=8, layer=False, kind="noise"), r.values)
    ow, ob, td = sc.layer("istft.refuse", 2, S)
    with pytest.raises(_lib.DiffsepError, match="output layer"):
        run_inv(r, x, S, T, lay=(ow[:, :2 * S - 1].contiguous(), ob, td), check_name=False)
    run_inv(r, x, S, T, lay=(ow[:, :2 * S].contiguous(), ob, td))      # exactly 2 S input channels is the narrowest layer


# ------------------------------------------------------------------------------------------------ round trip
@pytest.mark.parametrize("r", FUSED, ids=ROUTE_IDS[:2])
def test_fused_round_trip_within_the_sum_of_both_bounds(r):
    # fused STFT -> fused iSTFT of the sources' channels.  |back - want| <= the inverse bound on the spectrogram the device produced
    # + the forward bound carried through the inverse transform (istft_ref's dx: decompression by its mean-value bound, then |inv|).
    T, S, W = 3714, 2, 64
    xt, mix = sc.signal("stft.rt", 2, S, T)
    fwd = sc.stft_ref(xt, mix, W)
    sel = lambda t: torch.cat([t[..., 0:S], t[..., S + 1:2 * S + 1], torch.zeros_like(t[..., :8 - 2 * S])], -1)
    want = sc.istft_ref(sel(fwd["y"]), S, T, dx=sel(sc.stft_bound(fwd, "fused", r.dt)))
    spec = sel(run_fwd(r, xt, mix, W))
    got = sc.istft_ref(spec, S, T)
    back = run_inv(r, spec, S, T)
    bound = sc.istft_bound(got, "fused") + (1 + 2.0 ** -10) * want["Eola"] / want["env"]
    ratio = sc.worst_ratio(back, want["out"], bound)
    print(f"\n[round trip {r.id}] err / bound {ratio:.3f}, rel rms against the signal {sc.rel_rms(back, xt):.2e}")
    assert ratio < 1.0
    assert bool(((want["out"] - xt.double()).abs() <= 1e-9).all()), "the float64 references invert each other"


def test_the_cases_reach_every_instantiation():
    # from the case lists and the names every case asserts: all fused instantiations, the pack kernel in its three types, and the
    # three-launch inverse route on fp32, bfloat16 and half tensors (its unpack kernel's type is the tensor's)
    fwd = {fwd_name(r, FWD[cid]["S"]) for cid in FWD for r in ROUTES}
    assert fwd == {f"stft_fused_kernel<{n}>" for n in (2, 3, 4)} | {f"stft_pack_kernel<{t}>" for t in ("f32", "bf16", "f16")}
    inv = {inv_name(r, INV[cid]["S"], INV[cid]["exponent"]) for cid, r in INV_PAIRS}
    assert inv == {f"istft_fused_kernel<{ns},{em}>" for ns in (1, 2) for em in (0, 1, 2)} | {"istft_ola_kernel"}
