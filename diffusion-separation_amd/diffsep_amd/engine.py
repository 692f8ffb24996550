"""Engine: the Python handle on one device-resident NCSN++ score model + PC sampler.

PyTorch is used for device memory (tensor.data_ptr()), streams and nothing else: every FLOP of
the path runs in libdiffsep_hip.so.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import F32, BF16, F16, _ptr, _stream_ptr, call, check, lib


def _c_cfg(cfg):
    """the C-side view of a model config: the Python-only dtype code F16 is code 1 (16-bit storage) of the f16 build"""
    if cfg.dtype != F16:
        return cfg
    c2 = _lib.ModelConfig()
    C.memmove(C.byref(c2), C.byref(cfg), C.sizeof(cfg))
    c2.dtype = BF16
    return c2


def param_table(cfg):
    """[(name, shape, offset)] in the canonical (reference state_dict) order."""
    l = lib()
    cfg = _c_cfg(cfg)
    n = l.diffsep_param_count(C.byref(cfg))
    if n < 0:
        check(1)
    out = []
    name = C.create_string_buffer(256)
    shape = (C.c_int64 * 4)()
    ndim = C.c_int32()
    off = C.c_int64()
    for i in range(n):
        call(l, "diffsep_param_info", C.byref(cfg), i, name, 256, shape, C.byref(ndim), C.byref(off))
        out.append((name.value.decode(), tuple(int(shape[k]) for k in range(ndim.value)), int(off.value)))
    return out


def pack_state_dict(cfg, state, prefix=""):
    """Flatten {name: array/tensor} into the float32 blob the engine expects. Missing keys raise."""
    total = lib().diffsep_param_total(C.byref(_c_cfg(cfg)))
    blob = np.empty(total, dtype=np.float32)
    for name, shape, off in param_table(cfg):
        key = prefix + name
        if key not in state:
            raise KeyError(f"checkpoint is missing parameter '{key}'")
        v = state[key]
        v = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        if tuple(v.shape) != shape:
            raise ValueError(f"parameter '{key}' has shape {tuple(v.shape)}, expected {shape}")
        blob[off:off + v.size] = v.astype(np.float32, copy=False).reshape(-1)
    return blob


class SamplerTrace:
    """What a traced Engine.pc_sample leaves behind: steps (the snapshot steps), x / x_mean [len(steps),B,S,T] (one buffer
    each; x_mean None when not kept) and gram [N+1,B,3,S,S] float64 (None without a target), all on the device."""

    def __init__(self, steps, x, x_mean, gram):
        self.steps, self.x, self.x_mean, self.gram = list(steps), x, x_mean, gram

    def intermediates(self):
        """[(xt, xt_mean)] of the snapshot steps, views of the two buffers: the reference's `intermediate` list"""
        return [(self.x[k], self.x_mean[k] if self.x_mean is not None else None) for k in range(len(self.steps))]

    @staticmethod
    def cat(traces):
        """the traces of the minibatches of one batch, joined along the batch"""
        t0 = traces[0]
        return SamplerTrace(t0.steps, torch.cat([t.x for t in traces], dim=1),
                            None if t0.x_mean is None else torch.cat([t.x_mean for t in traces], dim=1),
                            None if t0.gram is None else torch.cat([t.gram for t in traces], dim=1))


class Engine:
    """Owns the repacked weights and workspace on the current CUDA(HIP) device."""

    def __init__(self, cfg, weights_blob, device=None, lib_kind=None):
        """lib_kind: which build of the library creates the engine ("bf16" / "f16"); default = by dtype (F16 lives in the
        half-precision build, everything else in the default one).  The fp32 engines are the same in both builds: pass
        lib_kind="f16" for a split / fp32 engine that serves as the head engine of an F16 one (pc_sample(tail=...))."""
        if not torch.cuda.is_available():
            raise _lib.DiffsepError("no GPU visible: the separation engine has no CPU path")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        # dtype F16 = the 16-bit engine (code 1) of the half-precision build of the library
        self.kind = _lib.half_kind(cfg.dtype) if lib_kind is None else lib_kind
        if cfg.dtype in (F16, BF16) and self.kind != _lib.half_kind(cfg.dtype):
            raise _lib.DiffsepError("a 16-bit engine lives in the library build of its storage format")
        self._L = lib(self.kind)
        cfg = _c_cfg(cfg)
        self.cfg = cfg
        blob = np.ascontiguousarray(weights_blob, dtype=np.float32)
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            call(self._L, "diffsep_engine_create", C.byref(cfg), blob.ctypes.data_as(C.c_void_p), blob.size, C.byref(self._h))
        self.S = cfg.num_sources

    def close(self):
        if getattr(self, "_h", None):
            self._L.diffsep_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def dtype(self):
        return self.cfg.dtype

    def device_bytes(self):
        return int(self._L.diffsep_engine_device_bytes(self._h))

    def set_graph(self, enable):
        call(self._L, "diffsep_engine_set_graph", self._h, int(bool(enable)))

    def set_option(self, name, value):
        """diffsep_engine_set_option.  Kernel-dispatch switches (0 / 1; A/B and test aids, the defaults are what ships; the
        table of DESIGN.md section 7b says which route each one closes): "no_rw", "no_rw128", "no_rw_res", "rw_small",
        "no_sw", "no_sw_rw", "no_sw_rows4", "sw_rows4", "no_sws", "no_wfrag", "no_attn_fused", "no_split256";
        "no_rw_helper" (the 64 -> 64 GroupNorm launches of the register-weight kernel without helper waves: same bits); launch
        geometry of the register-weight kernel: "rw_half", "rw_quarter", "rw_big_half" ("no_stft_fused" is a process
        default only: diffsep_set_option).  Others: "graph_cache" (captured graphs kept, LRU), "ablate" (measurement aid),
        "track_tensors", "trace" (debug_trace), "dbg_alloc".  Synchronises the device, drops the captured graphs (the three
        debug switches do neither)."""
        call(self._L, "diffsep_engine_set_option", self._h, str(name).encode(), int(value))

    def get_option(self, name):
        return int(self._L.diffsep_engine_get_option(self._h, str(name).encode()))

    CONV_CLASSES = ("conv3x3_8x32xN64", "conv3x3_8x32xN32", "conv3x3_8x8xN64", "gemm1x1_256xN64", "gemm1x1_256xN32",
                    "gemm1x1_64xN64", "conv3x3_ws_64to64", "conv3x3_small_16couts", "conv3x3_rw_regweights", "attention_fused",
                    "conv3x3_sw_streamed", "conv3x3_sws_split")

    def profile_begin(self):
        call(self._L, "diffsep_engine_profile_begin", self._h)

    def profile_end(self):
        """{class: (algorithmic flops, milliseconds, launches, algorithmic bytes)} of the MFMA kernels since
        profile_begin."""
        nc = len(self.CONV_CLASSES)
        fl, ms, n, by = (C.c_double * nc)(), (C.c_double * nc)(), (C.c_int64 * nc)(), (C.c_double * nc)()
        nw = C.c_int32(0)
        call(self._L, "diffsep_engine_profile_end_n", self._h, nc, fl, ms, n, by, C.byref(nw))
        return {k: (fl[i], ms[i], int(n[i]), by[i]) for i, k in enumerate(self.CONV_CLASSES[:nw.value])}

    def profile_records(self):
        """The launches of the last profile_begin .. profile_end span, one dict per launch: kernel instantiation (real
        template arguments), shape, algorithmic flops / bytes, milliseconds."""
        n = C.c_int32(0)
        call(self._L, "diffsep_engine_profile_records", self._h, None, 0, C.byref(n))
        buf = (_lib.ProfRecord * max(1, n.value))()
        call(self._L, "diffsep_engine_profile_records", self._h, buf, n.value, C.byref(n))
        return [dict(kernel=r.kernel.decode(), B=r.B, H=r.H, W=r.W, Cin=r.Cin, Cout=r.Cout, taps=r.taps,
                     skip_cin=r.skip_cin, has_res=bool(r.has_res), cls=r.cls, flops=r.flops, bytes=r.bytes, ms=r.ms)
                for r in buf[:n.value]]

    def padded_frames(self, T):
        return int(self._L.diffsep_padded_frames(C.byref(self.cfg), T))

    def bucket_length(self, W):
        """The longest signal whose padded frame count is W = 64 k: F = 1 + (T + n_fft - hop) // hop <= W.  Mixed-length
        batches padded to this length share ONE workspace plan / captured graph per (B, W), whatever their members'
        lengths (the results do not depend on the padding: diffsep_sampler_ext.lengths_host)."""
        return int(self.cfg.hop) * int(W) - (int(self.cfg.n_fft) - int(self.cfg.hop)) - 1

    def _f32(self, t):
        assert t.is_cuda and t.dtype == torch.float32, "device float32 tensor expected"
        return t.contiguous()

    def score(self, xt, t, mix):
        """score_fn(x, t, mix) -> [B,S,T]   (DiffSepModel.forward / ScoreModelNCSNpp.forward)."""
        xt, t, mix = self._f32(xt), self._f32(t), self._f32(mix)
        B, S, T = xt.shape
        assert S == self.S and mix.shape == (B, 1, T) and t.shape == (B,)
        out = torch.empty_like(xt)
        with torch.cuda.device(self.device):
            call(self._L, "diffsep_score_forward", self._h, _ptr(xt), _ptr(t), _ptr(mix), _ptr(out), B, T,
                 _stream_ptr(self.device))
        return out

    def reserve(self, B, T):
        """Size the workspace for batches of up to B x T samples now (later, smaller plans never reallocate)."""
        with torch.cuda.device(self.device):
            call(self._L, "diffsep_engine_reserve", self._h, int(B), int(T), _stream_ptr(self.device))

    def debug_absmax(self):
        """[(max finite |value|, non-finite count, rows H, channels C)] of every activation tensor of the last eager forward
        (set_option("track_tensors", 1) first; score() is an eager forward).  Debug / test aid."""
        n = C.c_int32(0)
        call(self._L, "diffsep_engine_debug_absmax", self._h, None, 0, C.byref(n))
        buf = (C.c_double * (4 * max(1, n.value)))()
        call(self._L, "diffsep_engine_debug_absmax", self._h, buf, n.value, C.byref(n))
        return [(buf[4 * i], int(buf[4 * i + 1]), int(buf[4 * i + 2]), int(buf[4 * i + 3])) for i in range(n.value)]

    def debug_arena(self):
        """(uint8 view of the workspace arena, offset of the forward region): every intermediate tensor of the last
        forward, in launch order.  Debug / test aid."""
        base, nb, fb = C.c_void_p(), C.c_int64(), C.c_int64()
        call(self._L, "diffsep_engine_debug_arena", self._h, C.byref(base), C.byref(nb), C.byref(fb))

        class _Raw:
            __cuda_array_interface__ = {"shape": (nb.value,), "typestr": "|u1", "data": (base.value, False), "version": 2}
        return torch.as_tensor(_Raw(), device=f"cuda:{self.device.index or 0}" if hasattr(self.device, "index") else "cuda"), fb.value

    def debug_trace(self):
        """[dict] of diffsep_engine_debug_trace: one record per tensor or side array the last eager forward wrote
        (set_option("trace", 1) first), in launch order: kind, role, kernel, mod, B, H, W, C, ld, f32, offset (bytes into the
        arena, -1: the caller's buffer) and stats (ABSOLUTE arena offset in bytes of the [B,C,2] int64 accumulators, or -1).
        Debug / test aid; trace_view / trace_stats turn a record into tensors."""
        n = C.c_int32(0)
        call(self._L, "diffsep_engine_debug_trace", self._h, None, None, 0, C.byref(n))
        nf, nb = _lib.TRACE_FIELDS, _lib.TRACE_NAME_BYTES
        fields = (C.c_int64 * (nf * max(1, n.value)))()
        names = C.create_string_buffer(nb * max(1, n.value))
        call(self._L, "diffsep_engine_debug_trace", self._h, fields, names, n.value, C.byref(n))
        raw = names.raw
        text = lambda i, lo, hi: raw[nb * i + lo:nb * i + hi].split(b"\0", 1)[0].decode()
        keys = ("mod", "B", "H", "W", "C", "ld", "f32", "offset", "stats")
        out = []
        for i in range(n.value):
            r = dict(zip(keys, (int(v) for v in fields[nf * i:nf * (i + 1)])), kind=text(i, 0, 16), role=text(i, 16, 32), kernel=text(i, 32, nb))
            r["f32"] = bool(r["f32"])
            out.append(r)
        return out

    def storage_dtype(self):
        """torch type of the engine's activation tensors"""
        if self.cfg.dtype != BF16:
            return torch.float32
        return torch.float16 if self.kind == "f16" else torch.bfloat16

    def trace_view(self, rec, arena=None):
        """a record of debug_trace() as a tensor [B,H,W,C] on the arena (no copy; the leading dimension becomes a stride)"""
        arena = self.debug_arena()[0] if arena is None else arena
        dt = torch.float32 if rec["f32"] else self.storage_dtype()
        esz = torch.empty((), dtype=dt).element_size()
        assert rec["offset"] >= 0 and rec["offset"] % esz == 0, "the record's tensor is not in the arena"
        n = rec["B"] * rec["H"] * rec["W"] * rec["ld"]
        flat = arena[rec["offset"]:rec["offset"] + n * esz].view(dt)
        return flat.view(rec["B"], rec["H"], rec["W"], rec["ld"])[..., :rec["C"]]

    def trace_stats(self, rec, arena=None):
        """the int64 GroupNorm accumulators [B,C,2] of a record (sum * 2^24, sum of squares * 2^16), a view of the arena"""
        arena = self.debug_arena()[0] if arena is None else arena
        assert rec["stats"] >= 0 and rec["stats"] % 8 == 0, "the record has no accumulators"
        n = rec["B"] * rec["C"] * 2
        return arena[rec["stats"]:rec["stats"] + n * 8].view(torch.int64).view(rec["B"], rec["C"], 2)

    def backbone(self, x_nhwc, t):
        """NCSNpp.forward on a packed NHWC input [B,256,W,Cpad] (engine dtype storage)."""
        B, H, W, Cp = x_nhwc.shape
        t = self._f32(t)
        cout = ((2 * self.S + 7) // 8) * 8
        y = torch.zeros((B, H, W, cout), dtype=x_nhwc.dtype, device=x_nhwc.device)
        with torch.cuda.device(self.device):
            call(self._L, "diffsep_backbone_forward", self._h, _ptr(x_nhwc.contiguous()), _ptr(t), _ptr(y), B, W,
                 _stream_ptr(self.device))
        return y

    def _ext_arrays(self, ext, B, lengths, seeds):
        """lengths / seeds -> the host-pointer fields of a SamplerExt or OdeExt; returns the arrays they refer to, which the
        caller keeps alive until its library call has returned"""
        keep = []
        for name, v, dt in (("lengths", lengths, np.int64), ("seeds", seeds, np.uint64)):
            if v is not None:
                arr, ptr = _lib.host_array(v, dt, B, name)
                setattr(ext, name + "_host", ptr)
                keep.append(arr)
        return keep

    def _sampler_ext(self, B, lengths, seeds, tail, tail_steps, head_steps):
        """(SamplerExt or None when the call uses no extension, the host arrays to keep alive)"""
        hybrid = tail is not None and (tail_steps > 0 or head_steps > 0)
        if lengths is None and seeds is None and not hybrid:
            return None, []
        ext = _lib.SamplerExt()
        keep = self._ext_arrays(ext, B, lengths, seeds)
        if hybrid:
            if tail.kind != self.kind:  # an engine handle means something to the library that created it only
                raise _lib.DiffsepError(f"the other engine was created by the '{tail.kind}' build of the library, this one "
                                        f"by the '{self.kind}' build: create it with Engine(..., lib_kind='{self.kind}')")
            ext.tail_engine, ext.tail_steps, ext.head_steps = tail._h, int(tail_steps), int(head_steps)
        return ext, keep

    def _state_args(self, B, T, x_init, noise):
        """x_init / noise [B,S,T] as the library takes them (None stays None)"""
        for name, v in (("x_init", x_init), ("noise", noise)):
            if v is not None:
                assert tuple(v.shape) == (B, self.S, T), f"{name} must be [B,S,T]"
        return (self._f32(x_init) if x_init is not None else None), (self._f32(noise) if noise is not None else None)

    def pc_sample(self, mix_norm, sde, N=30, corrector_steps=1, snr=0.5, eps=0.03, denoise=True,
                  predictor="reverse_diffusion", corrector="ald2", noise=None, seed=0, timesteps=None, lengths=None,
                  seeds=None, tail=None, tail_steps=0, head_steps=0, snapshots=None, snapshot_means=True, target=None,
                  x_init=None, first_step=0, last_step=None):
        """The whole sampler (sdes.get_pc_sampler(...)()).  sde: dict(kind, ndim, d_lambda, sigma_min, sigma_max).
        Tracing (diffsep_pc_sample_trace; with snapshots or target the result is (out, nfe, trace), a SamplerTrace):
        snapshots = the reverse steps whose state (x, and x_mean unless snapshot_means=False) is kept, as the reference's
        intermediate=True appends it between corrector and predictor — a strictly ascending list of steps in [0, N) (the
        library refuses anything else) or "all"; target [B,S,T] (zero beyond each utterance's length) = also the Gram sums of every step's state, and last of
        the result, against it: trace.gram [N+1,B,3,S,S] float64, row i bit for bit ops.gram(target, trace.x[i]).
        Extensions (diffsep_sampler_ext): lengths [B] = a zero-padded batch of utterances of different lengths that share
        one padded frame count; seeds [B] = per-utterance device-RNG seeds; tail / head_steps / tail_steps = evaluate the
        score of the FIRST head_steps and / or the last tail_steps reverse steps on another Engine (dtype "hybrid" of
        pl_model: a split-fp32 engine for the first HYBRID_HEAD_STEPS steps of a 16-bit one — the early steps carry
        the rounding error).
        Both ends open (diffsep_pc_sample_from): x_init [B,S,T] = the state to start from instead of the
        prior sample (ops.warm_start builds one from another separator's estimates); only the reverse steps
        [first_step, last_step) of the N-point grid run (last_step None = N; first_step > 0 needs x_init), each at its own time
        ts[i], with dt = 1/N and its own draws of `noise` (always the full [draws,B,S,T]) or of the device RNG, so that
        pc_sample(last_step=k) followed by pc_sample(x_init=<its result>, first_step=k) is bit for bit the full call.  With
        last_step < N the result is the state x whatever denoise says; nfe counts the executed steps; snapshots lie in the
        range, "all" means all of it, and of trace.gram only the rows of executed steps (and row N with last_step = N) are written."""
        mix_norm = self._f32(mix_norm)
        B, one, T = mix_norm.shape
        assert one == 1
        sc = _lib.sde_config(sde)
        sm = _lib.SamplerConfig(N, corrector_steps, snr, eps, int(bool(denoise)), _lib.PREDICTORS[predictor],
                                _lib.CORRECTORS[corrector])
        out = torch.empty((B, self.S, T), dtype=torch.float32, device=mix_norm.device)
        if noise is not None:
            noise = self._f32(noise)
            ncs = corrector_steps if corrector != "none" else 0
            npred = 1 if predictor != "none" else 0
            assert noise.shape == (1 + N * (ncs + npred), B, self.S, T), "noise must be [draws,B,S,T]"
        ts = None
        if timesteps is not None:
            ts = np.ascontiguousarray(timesteps, dtype=np.float32)
            assert ts.size >= N
        nfe = C.c_int32()
        ext, keep = self._sampler_ext(B, lengths, seeds, tail, tail_steps, head_steps)  # (keep: alive until this returns)
        ranged =x_init is not None or first_step != 0 or last_step is not None
        first, last = int(first_step), int(N if last_step is None else last_step)
        if x_init is not None:
            x_init = self._f32(x_init)
            assert tuple(x_init.shape) == (B, self.S, T), "x_init must be [B,S,T]"
        if ranged and (last_step == 0 or not 0 <= first < last <= N):  # (0 means N to the library: an empty range is refused here)
            raise _lib.DiffsepError(f"pc_sample: the step range must satisfy 0 <= first_step < last_step <= N, got [{first}, {last}) of {N}")
        tail_args = (_ptr(x_init), first, last, _stream_ptr(self.device)) if ranged else (_stream_ptr(self.device),)
        if snapshots is None and target is None:
            with torch.cuda.device(self.device):
                if ranged:
                    call(self._L, "diffsep_pc_sample_from", self._h, C.byref(sc), C.byref(sm), C.byref(ext) if ext is not None else None,
                         _ptr(mix_norm), _ptr(out), B, T, _ptr(noise), seed, ts.ctypes.data_as(C.c_void_p) if ts is not None else None,
                         C.byref(nfe), 0, None, None, None, None, None, *tail_args)
                    return out, int(nfe.value)
                call(self._L, "diffsep_pc_sample_ex", self._h, C.byref(sc), C.byref(sm), C.byref(ext) if ext is not None else None,
                     _ptr(mix_norm), _ptr(out), B, T, _ptr(noise), seed, ts.ctypes.data_as(C.c_void_p) if ts is not None else None,
                     C.byref(nfe), _stream_ptr(self.device))
            return out, int(nfe.value)
        steps = list(range(first, last)) if isinstance(snapshots, str) and snapshots == "all" else [int(s) for s in (snapshots or [])]
        n_snap = len(steps)
        dev = mix_norm.device
        snap_x = torch.empty((n_snap, B, self.S, T), dtype=torch.float32, device=dev)
        snap_xm = torch.empty_like(snap_x) if (snapshot_means and n_snap) else None
        gram = None
        if target is not None:
            target = self._f32(target)
            assert tuple(target.shape) == (B, self.S, T), "target must be [B,S,T]"
            gram = torch.empty((N + 1, B, 3, self.S, self.S), dtype=torch.float64, device=dev)
            if first > 0 or last < N:  # (the rows of steps that do not run are not written: NaN marks them)
                gram.fill_(float("nan"))
        sa_ = np.ascontiguousarray(steps, dtype=np.int32)
        with torch.cuda.device(self.device):
            call(self._L, "diffsep_pc_sample_from" if ranged else "diffsep_pc_sample_trace", self._h, C.byref(sc), C.byref(sm),
                 C.byref(ext) if ext is not None else None,
                 _ptr(mix_norm), _ptr(out), B, T, _ptr(noise), seed, ts.ctypes.data_as(C.c_void_p) if ts is not None else None,
                 C.byref(nfe), n_snap, sa_.ctypes.data_as(C.POINTER(C.c_int32)), _ptr(snap_x) if n_snap else None,
                 _ptr(snap_xm), _ptr(target), _ptr(gram), *tail_args)
        return out, int(nfe.value), SamplerTrace(steps, snap_x, snap_xm, gram)

    def _ode_setup(self, mix_norm, sde, method, rtol, atol, eps, first_step, max_step, max_nfe, denoise, N, x_init, noise):
        """what both ODE entries make of their arguments: (mix_norm, SdeConfig, OdeConfig, x_init, noise, out)"""
        if method not in _lib.ODE_METHODS:
            raise NotImplementedError(f"ODE method '{method}': only RK45 and RK23 run on the engine")
        mix_norm = self._f32(mix_norm)
        B, one, T = mix_norm.shape
        assert one == 1
        sc = _lib.sde_config(sde)
        oc = _lib.OdeConfig(float(rtol), float(atol), float(eps), float(first_step or 0.0),
                            float(max_step) if max_step is not None else 0.0, _lib.ODE_METHODS[method], int(max_nfe or 0),
                            int(bool(denoise)), int(N))
        x_init, noise = self._state_args(B, T, x_init, noise)
        out = torch.empty((B, self.S, T), dtype=torch.float32, device=mix_norm.device)
        return mix_norm, sc, oc, x_init, noise, out

    def ode_sample(self, mix_norm, sde, method="RK45", rtol=1e-5, atol=1e-5, eps=3e-2, first_step=None, max_step=None,
                   max_nfe=0, denoise=True, N=30, x_init=None, noise=None, seed=0, lengths=None, tail=None):
        """The probability-flow ODE sampler (sdes.get_ode_sampler(...)(), diffsep_ode_sample): scipy's RK45 / RK23
        controller on the device-resident state, the whole batch as one system.  x_init [B,S,T]: start from this x_T (the
        reference's z); else the prior sample from noise [B,S,T] or from the device RNG keyed by seed.  Returns
        (out [B,S,T], info dict: nfev, n_accepted, n_rejected, status 0 / -1 / 1, t_final)."""
        if lengths is not None:
            raise _lib.DiffsepError("ode_sample: the whole batch is one ODE system with one step size; mixed-length "
                                    "batches are not supported (run the utterances one by one)")
        if tail is not None:
            raise _lib.DiffsepError("ode_sample: every evaluation runs on one engine; there is no tail engine")
        mix_norm, sc, oc, x_init, noise, out = self._ode_setup(mix_norm, sde, method, rtol, atol, eps, first_step, max_step,
                                                               max_nfe, denoise, N, x_init, noise)
        B, _, T = mix_norm.shape
        info = _lib.OdeInfo()
        with torch.cuda.device(self.device):
            call(self._L, "diffsep_ode_sample", self._h, C.byref(sc), C.byref(oc), _ptr(mix_norm), _ptr(x_init), _ptr(noise),
                 int(seed) % (1 << 64), _ptr(out), B, T, C.byref(info), _stream_ptr(self.device))
        return out, _lib.ode_info_dict(info)

    def ode_sample_each(self, mix_norm, sde, lengths=None, seeds=None, method="RK45", rtol=1e-5, atol=1e-5, eps=3e-2,
                        first_step=None, max_step=None, max_nfe=0, denoise=True, N=30, x_init=None, noise=None, seed=0):
        """The probability-flow ODE sampler with one step controller per utterance (diffsep_ode_sample_each): the batch
        is B independent systems solved in lock step, all sharing every network evaluation.  lengths [B]: a zero-padded
        batch of utterances that share one padded frame count; seeds [B]: per-utterance seeds of the prior draw.  Where the
        fp32 network evaluation does not depend on the batch row b inside lengths[b] is bit-for-bit
        ode_sample on that utterance alone with its seed.  Returns
        (out [B,S,T], [info dict per utterance], evals_run = network evaluations actually run = max nfev)."""
        mix_norm, sc, oc, x_init, noise, out = self._ode_setup(mix_norm, sde, method, rtol, atol, eps, first_step, max_step,
                                                               max_nfe, denoise, N, x_init, noise)
        B, _, T = mix_norm.shape
        ext = _lib.OdeExt()
        keep = self._ext_arrays(ext, B, lengths, seeds)  # (alive until this method returns)
        infos = (_lib.OdeInfo * B)()
        evals = C.c_int32()
        with torch.cuda.device(self.device):
            call(self._L, "diffsep_ode_sample_each", self._h, C.byref(sc), C.byref(oc), C.byref(ext), _ptr(mix_norm),
                 _ptr(x_init), _ptr(noise), int(seed) % (1 << 64), _ptr(out), B, T, infos, C.byref(evals),
                 _stream_ptr(self.device))
        return out, [_lib.ode_info_dict(i) for i in infos], int(evals.value)

    def ode_sample_fixed(self, mix_norm, sde, method="heun", steps=30, t_start=None, eps=3e-2, timesteps=None, denoise=True,
                         N=30, x_init=None, noise=None, seed=0, lengths=None, seeds=None, tail=None, head_steps=0,
                         tail_steps=0, want_err=False):
        """The probability-flow ODE on a fixed grid (diffsep_ode_sample_fixed): `steps` steps of "euler", "heun", "midpoint",
        "rk4" or "ab2" from t_start (None: 1.0) down to eps, or along timesteps (steps + 1 strictly descending times inside
        (0, 1]).  The whole solve is ENQUEUED on the current stream, like pc_sample: nothing is read back, the call does not
        block, and its cost is known beforehand (_lib.odef_nfe).  x_init / noise / seed / lengths / seeds as in pc_sample
        (a start below 1 needs x_init, e.g. from ops.warm_start); tail / head_steps / tail_steps: the evaluations of the
        first head_steps and last tail_steps SOLVER steps run on another Engine.  want_err (heun, midpoint, ab2): also the
        local-error trace, a device float64 tensor [steps,B,2] of (RMS of step minus embedded Euler step, RMS of y_i) per
        step and utterance, not read back here.  method "ddim" / "dpmpp2m" (diffsep_ode_sample_expint):
        the exponential integrators DDIM and DPM-Solver++ 2M on the same grid with the same arguments, `steps` network
        evaluations each; want_err (dpmpp2m): RMS of the step minus its DDIM step (an exact 0 at step 0), RMS of y_i.
        Returns (out [B,S,T], info: nfe, method, steps[, err])."""
        expint = method in _lib.EXPINT_METHODS  # "ddim" / "dpmpp2m": diffsep_ode_sample_expint, the same argument list
        if method not in _lib.ODEF_METHODS and not expint:
            raise NotImplementedError(f"ode_sample_fixed: method '{method}' (one of {sorted(_lib.ODEF_METHODS)} or "
                                      f"{sorted(_lib.EXPINT_METHODS)})")
        mix_norm = self._f32(mix_norm)
        B, one, T = mix_norm.shape
        assert one == 1
        M = int(steps)
        sc = _lib.sde_config(sde)
        x_init, noise = self._state_args(B, T, x_init, noise)
        ts = None
        if timesteps is not None:
            ts = np.ascontiguousarray(timesteps.detach().cpu().numpy() if hasattr(timesteps, "detach") else timesteps,
                                      dtype=np.float64).reshape(-1)
            if ts.size != M + 1:
                raise _lib.DiffsepError(f"ode_sample_fixed: timesteps must hold steps + 1 = {M + 1} times, got {ts.size}")
        ext, keep = self._sampler_ext(B, lengths, seeds, tail, tail_steps, head_steps)  # (keep: alive until this returns)
        out =torch.empty((B, self.S, T), dtype=torch.float32, device=mix_norm.device)
        err = torch.empty((max(M, 0), B, 2), dtype=torch.float64, device=mix_norm.device) if want_err else None
        nfe = C.c_int32()
        with torch.cuda.device(self.device):
            call(self._L, "diffsep_ode_sample_expint" if expint else "diffsep_ode_sample_fixed", self._h, C.byref(sc),
                 _lib.EXPINT_METHODS[method] if expint else _lib.ODEF_METHODS[method], M,
                 float(t_start) if t_start is not None else 0.0, float(eps), int(bool(denoise)), int(N),
                 C.byref(ext) if ext is not None else None, _ptr(mix_norm), _ptr(x_init), _ptr(noise), int(seed) % (1 << 64),
                 ts.ctypes.data_as(C.POINTER(C.c_double)) if ts is not None else None, _ptr(out), _ptr(err), B, T,
                 C.byref(nfe), _stream_ptr(self.device))
        info = dict(nfe=int(nfe.value), method=method, steps=M)
        if want_err:
            info["err"] = err
        return out, info
