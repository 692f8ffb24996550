#!/usr/bin/env python3
"""Per-phase cycle counters of the kernels that carry PT_MARKs (csrc/phase_timing.h), read from a profiling variant of the library:

    make -C diffusion-separation_amd/csrc -j16 variant NAME=conv3x3_rw_timing SRC=conv3x3_rw VFLAGS=-DRW_TIMING
    python tools/phase_timing.py --kernel conv3x3_rw --lib diffusion-separation_amd/ab/libdiffsep_hip_conv3x3_rw_timing.so

One table (KERNELS), one measure loop (2 warm-up runs, reset, 5 timed runs between events, read), one printer.
--cases: a substring of the case labels, or, for the kernels whose entry says so, an explicit list "a,b,c;a,b,c".
The library's dispatch switches and the halo kernels' launch hooks are environment variables as everywhere else
(DIFFSEP_NO_RW=1, DIFFSEP_NO_SW=1, ...: csrc/engine.hip; DIFFSEP_<RW | SW | SWS>_G, DIFFSEP_<..>_DBG: csrc/conv3x3_halo.h)."""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = 5  # timed runs per case

HALO = ["prologue: staging of the first chunk", "barrier wait", "3x3 chunk phases", "skip chunk phases", "epilogue", "tail (statistics)",
        "prologue: tables + descriptors", "prologue: first loads + weight fragments issued, barrier"]
SW = HALO[:4] + ["final epilogue", "tail (statistics)", "prologue: tables + descriptors", "prologue: first loads issued, tables, barrier"]
RW_HELPER = ["helper: up to the tables", "helper: first chunk", "helper: waiting at phase barriers", "helper: staging", "-", "-",
             "prologue: tables + descriptors"]  # (slot 6: the prologue every wave runs before the roles part)
CONV = ["setup (offsets, descriptors)", "issue first loads", "wait first loads", "activation of chunk 0", "barrier+LDS store+barrier",
        "issue next loads", "MFMA loop (+activation of next)", "acc dump+barriers+residual loads", "epilogue LDS read+math",
        "epilogue global stores", "statistics reduce"]


def _explicit(spec, n):
    """'a,b;c,d' -> [(a, b), (c, d)] if spec is such a list of n-tuples (or n + 1), else None (spec is a label filter)."""
    try:
        rows = [tuple(int(v) for v in c.split(",")) for c in spec.split(";")] if spec else None
    except ValueError:
        return None
    return rows if rows and all(len(r) in (n, n + 1) for r in rows) else None


def _conv_cases(spec):
    """(k, cin, cout, H, W); explicit --cases "k,cin,cout,H,W;...".  The 16-bit launches, then the split engine's."""
    import torch
    from diffsep_amd import ops
    B, cases = 16, []

    def bf16(k, ci, co, H, W):
        def make():
            x = torch.randn(B, H, W, ci, device="cuda").to(torch.bfloat16)
            w = (torch.randn(co, k * k, ci, device="cuda") / (k * k * ci) ** 0.5).to(torch.bfloat16)
            b = torch.randn(co, device="cuda")
            sc, sh = torch.rand(B, ci, device="cuda") + 0.5, torch.randn(B, ci, device="cuda") * 0.1
            res = torch.randn(B, H, W, co, device="cuda").to(torch.bfloat16)
            return lambda: ops.conv2d_fused(x, w, b, co, k, gn=(sc, sh), gn_act=1, res=res, out_scale=0.7071)
        return f"k{k} {ci}->{co} {H}x{W}", make

    def f32(k, ci, co, H, W, split):
        def make():
            x = torch.randn(B, H, W, ci, device="cuda")
            w = ops.pack_conv_weight(torch.randn(co, ci, k, k) / (k * k * ci) ** 0.5, torch.float32, chunk=16).cuda()
            b = torch.randn(co, device="cuda")
            sc, sh = torch.rand(B, ci, device="cuda") + 0.5, torch.randn(B, ci, device="cuda") * 0.1
            res, y = torch.randn(B, H, W, co, device="cuda"), torch.zeros(B, H, W, co, device="cuda")
            return lambda: ops.conv2d_fused(x, w, b, co, k, gn=(sc, sh), gn_act=1, res=res, out_scale=0.7071, out=y, w_chunk=16, split=split)
        return f"k{k} {ci}->{co} {H}x{W} f32 split={split}", make

    rows = _explicit(spec, 5)
    if rows:
        return [bf16(*r[:5]) for r in rows]
    cases = [bf16(3, 128, 64, 256, 256), bf16(3, 128, 128, 64, 64), bf16(3, 256, 128, 32, 32)]
    return cases + [f32(3, 64, 64, 256, 256, True), f32(3, 64, 64, 256, 256, False), f32(3, 128, 128, 64, 64, True)]


def _ws_cases(spec):
    import torch
    from diffsep_amd import ops

    def make():
        B, ci, co, k, H, W = 16, 64, 64, 3, 256, 256
        x = torch.randn(B, H, W, ci, device="cuda").to(torch.bfloat16)
        w = (torch.randn(co, 9, ci, device="cuda") / 24).to(torch.bfloat16)
        b = torch.randn(co, device="cuda")
        sc, sh = torch.rand(B, ci, device="cuda") + 0.5, torch.randn(B, ci, device="cuda") * 0.1
        res = torch.randn(B, H, W, co, device="cuda").to(torch.bfloat16)
        y = torch.zeros(B, H, W, co, device="cuda", dtype=torch.bfloat16)
        _, st = ops.conv2d_fused(x, w, b, co, k, out=y, stats=True)
        return lambda: ops.conv2d_fused(x, w, b, co, k, gn=(sc, sh), gn_act=1, res=res, out_scale=0.7071, out=y, stats=st)
    return [("64->64 256x256 GN+SiLU+stats+residual", make)]


def _small_cases(spec):
    import torch
    from diffsep_amd import ops

    def case(ci, co, H, W, act):
        def make():
            B = 16
            x = torch.randn(B, H, W, ci, device="cuda").to(torch.bfloat16)
            w = ops.pack_conv_weight(torch.randn(co, ci, 3, 3) / (9 * ci) ** 0.5, torch.bfloat16, chunk=32).cuda()
            b = torch.randn(co, device="cuda")
            sc, sh = torch.rand(B, ci, device="cuda") + 0.5, torch.randn(B, ci, device="cuda") * 0.1
            res = torch.randn(B, H, W, co, device="cuda").to(torch.bfloat16)
            st = torch.zeros(B, co, 2, dtype=torch.int64, device="cuda")
            y = torch.zeros(B, H, W, co, device="cuda", dtype=torch.bfloat16)
            kw = dict(gn=(sc, sh), gn_act=1) if act else {}
            return lambda: ops.conv2d_fused(x, w, b, co, 3, res=res, out_scale=0.7071, w_chunk=32, out=y, stats=st, **kw)
        return f"{ci}->{co} {H}x{W} act={act}", make
    return [case(128, 128, 16, 16, 1), case(128, 128, 16, 16, None), case(128, 128, 8, 8, 1), case(128, 128, 4, 4, 1), case(128, 128, 4, 4, None)]


def _attn_cases(spec):
    """In the engine: one nf = 64 score evaluation at B = 16 (three 16 x 16 blocks and the 4 x 4 bottleneck block)."""
    import torch
    from diffsep_amd import _lib, synth
    from diffsep_amd.engine import Engine, pack_state_dict, param_table

    def make():
        cfg = _lib.model_config(nf=64, num_sources=2, dtype=_lib.F16)
        eng = Engine(cfg, pack_state_dict(cfg, synth.synth_state_dict([(n, s) for n, s, _ in param_table(cfg)], 7)))
        eng.set_graph(False)
        B, T = 16, 32000
        x, t, mix = torch.randn(B, 2, T, device="cuda") * 0.3, torch.full((B,), 0.5, device="cuda"), torch.randn(B, 1, T, device="cuda")
        return lambda: eng.score(x, t, mix)
    return [("engine nf=64 B=16 T=32000: 4 attention blocks per evaluation (average over the 16x16 and 4x4 blocks)", make)]


def _stft_cases(spec):
    import torch
    from diffsep_amd import ops
    B, S, T, W = 16, 2, 32000, 256

    def fwd():
        x = torch.randn(B, S + 1, T, device="cuda") * 0.3
        xt, mix = x[:, :S].contiguous(), x[:, S:].contiguous()
        return lambda: ops.stft_pack(xt, mix, W, 8, shift=True, dtype=torch.float16)

    def inv():
        yy = (torch.randn(B, 256, W, 8, device="cuda") * 0.2).half()
        return lambda: ops.istft_unpack(yy, S, T)
    return [("stft_fused B=16 S=2 T=32000 (phases 0-2)", fwd), ("istft_fused B=16 S=2 T=32000 (phases 4-7)", inv)]


def _rw_cases(dtype_name):
    """(cin, cout, H, W, fused[, B]); explicit --cases "cin,cout,H,W,fused[,B];..." (fused: 0 plain, 1 Conv_0, 2 Conv_1 + residual)."""
    def cases(spec):
        import torch
        from diffsep_amd import ops
        DT = getattr(torch, dtype_name)

        def case(ci, co, H, W, fused, B=16):
            def make():
                kc = 32  # chunk-major [Cin/32][9][Cout][32] like the engine's weights
                x = torch.randn(B, H, W, ci, device="cuda").to(DT)
                w = (torch.randn(co, 9, ci, device="cuda") / (9 * ci) ** 0.5).to(DT)
                w = w.reshape(co, 9, ci // kc, kc).permute(2, 1, 0, 3).contiguous()
                b = torch.randn(co, device="cuda")
                sc, sh = torch.rand(B, ci, device="cuda") + 0.5, torch.randn(B, ci, device="cuda") * 0.1
                res = torch.randn(B, H, W, co, device="cuda").to(DT)
                y = torch.zeros(B, H, W, co, device="cuda", dtype=DT)
                _, st = ops.conv2d_fused(x, w, b, co, 3, out=y, stats=True, w_chunk=kc)
                if fused == 2:    # Conv_1 of a plain block: GroupNorm + SiLU, bias, residual, 1/sqrt(2), statistics
                    return lambda: ops.conv2d_fused(x, w, b, co, 3, gn=(sc, sh), gn_act=1, res=res, out_scale=0.7071, out=y, stats=st, w_chunk=kc)
                if fused == 1:    # Conv_0: GroupNorm + SiLU, bias, statistics
                    return lambda: ops.conv2d_fused(x, w, b, co, 3, gn=(sc, sh), gn_act=1, out=y, stats=st, w_chunk=kc)
                return lambda: ops.conv2d_fused(x, w, b, co, 3, out=y, w_chunk=kc)
            return f"B={B} {ci}->{co} {H}x{W} {['plain', 'GN+SiLU+stats', 'GN+SiLU+stats+residual'][fused]}", make
        rows = _explicit(spec, 5) or [(64, 64, 256, 256, 2), (64, 64, 256, 256, 1), (64, 64, 256, 256, 0), (128, 64, 256, 256, 1),
                                      (128, 64, 256, 256, 0), (64, 64, 128, 128, 1)]
        return [case(*r) for r in rows]
    return cases


def _sw_cases(dtype_name):
    def cases(spec):
        import torch
        from diffsep_amd import ops
        DT, B, CO = getattr(torch, dtype_name), 16, 128
        pack = ops.pack_frag_weight_split if DT == torch.float32 else (lambda w: ops.pack_frag_weight(w, DT))

        def case(name, C1, C2, skip, H):
            def make():
                W, C = H, C1 + C2
                a = torch.randn(B, H, W, C1, device="cuda").to(DT)
                bt = torch.randn(B, H, W, C2, device="cuda").to(DT) if C2 else None
                wf = pack(torch.randn(CO, C, 3, 3) / (9 * C) ** 0.5).cuda()
                bias = torch.randn(CO, device="cuda")
                sc, sh = torch.rand(B, C, device="cuda") + 0.5, torch.randn(B, C, device="cuda") * 0.1
                sk = None
                if skip:
                    sk = (torch.randn(B, H, W, skip[0], device="cuda").to(DT), torch.randn(B, H, W, skip[1], device="cuda").to(DT),
                          pack(torch.randn(CO, sum(skip), 1, 1) / sum(skip) ** 0.5).cuda())
                y = torch.zeros(B, H, W, CO, device="cuda", dtype=DT)
                st = torch.zeros((B, CO, 2), dtype=torch.int64, device="cuda")
                return lambda: ops.conv3x3_streamed(a, wf, CO, x2=bt, gn=(sc, sh), bias=bias, skip=sk, stats=st, out=y)
            return name, make
        return [case("128->128 @256^2", 128, 0, None, 256), case("256->128 @256^2", 128, 128, None, 256),
                case("128->128 +skip256 @256^2", 128, 0, (128, 128), 256), case("256->128 @64^2", 128, 128, None, 64),
                case("128->128 @64^2", 128, 0, None, 64)]
    return cases


# source: under csrc/; macro: its -D<X>_TIMING; kind: which library the variant replaces; symbol: the read-back function;
# phases: names of counter slots 0 .. (per reporting row: rows[r] names row r's wave); cases(spec) -> [(label, make)],
# make() -> the callable that is timed; opts: process options set before the cases run
KERNELS = {
    "conv_mfma": dict(source="conv_mfma.hip", macro="CONV_TIMING", kind="bf16", symbol="diffsep_debug_read", phases=[CONV], rows=1, cases=_conv_cases),
    "conv3x3_ws": dict(source="conv3x3_ws.hip", macro="WS_TIMING", kind="bf16", symbol="diffsep_ws_debug_read", rows=2,
                       phases=[["barrier wait", "issue loads", "MFMA + activation", "LDS write", "prologue", "tail (stats)", "epilogue"]] * 2,
                       opts={"no_rw": 1}, cases=_ws_cases),  # (64 -> 64 at 256^2 is the register-weight kernel's by default)
    "conv3x3_small": dict(source="conv3x3_small.hip", macro="SM_TIMING", kind="bf16", symbol="diffsep_small_debug_read", rows=1,
                          phases=[["setup (geometry)", "issue loads of 2 phases", "GroupNorm table + fetch", "wait for the phase's loads", "activation",
                                   "barrier + LDS write + issue + barrier", "MFMA", "epilogue + store", "statistics"]], cases=_small_cases),
    "attn_fused": dict(source="attn_fused.hip", macro="ATTN_TIMING", kind="f16", symbol="diffsep_attn_debug_read", rows=1,
                       phases=[["issue: table operands, input tile, Wv + Wq fragments", "barrier 1 (table visible)", "affine + h -> LDS", "barrier 2",
                                "V^T product -> LDS", "barrier 3", "Q and Q' products", "S = Q' h^T", "softmax", "P V (+ Wo fragments)",
                                "output projection, residual, stores", "statistics"]], cases=_attn_cases),
    "stft": dict(source="stft.hip", macro="ST_TIMING", kind="f16", symbol="diffsep_st_debug_read", rows=1,
                 phases=[["stft: staging", "stft: products", "stft: epilogue", "-", "istft: U prologue", "istft: products", "istft: overlap-add stores",
                          "istft: envelope + output"]], cases=_stft_cases),
    "conv3x3_rw": dict(source="conv3x3_rw.hip", macro="RW_TIMING", kind="bf16", symbol="diffsep_rw_debug_read", rows=2, phases=[HALO, RW_HELPER],
                       opts={"rw_small": 1}, cases=_rw_cases("bfloat16")),
    "conv3x3_rw_f16": dict(source="conv3x3_rw.hip", macro="RW_TIMING", kind="f16", symbol="diffsep_rw_debug_read", rows=2, phases=[HALO, RW_HELPER],
                           opts={"rw_small": 1}, cases=_rw_cases("float16")),
    "conv3x3_rw4": dict(source="conv3x3_rw4.hip", macro="RW_TIMING", kind="bf16", symbol="diffsep_rw4_debug_read", rows=1, phases=[HALO],
                        opts={"rw_small": 1, "no_rw_helper": 1}, cases=_rw_cases("bfloat16")),
    "conv3x3_sw": dict(source="conv3x3_sw.hip", macro="SW_TIMING", kind="f16", symbol="diffsep_sw_debug_read", rows=1, phases=[SW], cases=_sw_cases("float16")),
    "conv3x3_sws": dict(source="conv3x3_sws.hip", macro="SWS_TIMING", kind="bf16", symbol="diffsep_sws_debug_read", rows=1, phases=[SW],
                        cases=_sw_cases("float32")),
}
ROW_NAMES = {"conv3x3_ws": ["wave 0 (group 0)", "wave 4 (group 1)"], "conv3x3_rw": ["wave 0 (matrix role)", "wave 4 (helper role)"],
             "conv3x3_rw_f16": ["wave 0 (matrix role)", "wave 4 (helper role)"]}


def make_line(name):
    e = KERNELS[name]
    tag = f"{name}_timing"
    so = f"diffusion-separation_amd/ab/libdiffsep_hip{'_f16' if e['kind'] == 'f16' else ''}_{tag}.so"
    return (f"make -C diffusion-separation_amd/csrc -j16 variant NAME={tag} SRC={e['source'][:-4]} VFLAGS=-D{e['macro']}"
            f"{' KIND=f16' if e['kind'] == 'f16' else ''}\n  python tools/phase_timing.py --kernel {name} --lib {so}")


def measure(read, run):
    """2 warm-up runs, reset, RUNS timed runs between events, read -> (us per run, the 32 counters)."""
    import torch
    out = (ctypes.c_ulonglong * 32)()
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    read(out, 1)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(RUNS):
        run()
    e1.record()
    torch.cuda.synchronize()
    read(out, 1)
    return e0.elapsed_time(e1) / RUNS * 1e3, list(out)


def print_table(name, label, us, out):
    e = KERNELS[name]
    print(f"{label}: {us:.1f} us per run")
    for r in range(e["rows"]):
        c, names = out[16 * r:16 * r + 16], e["phases"][r]
        nb, tot, wall = c[15], sum(c[:12]), c[14]
        if nb == 0:
            print(f"  row {r}: nothing reported" + (" (the launch took another route: DIFFSEP_NO_RW=1, DIFFSEP_NO_SW=1, ... select it)" if r == 0 else
                                                    " (this instantiation has no second reporting wave)"))
            continue
        clock = f", {wall / nb * 10:.0f} ns wall = {tot / (wall * 10):.2f} ticks/ns" if wall else ""
        print(f"  {ROW_NAMES.get(name, ['wave 0'])[r]}: {nb // RUNS} blocks per run, {tot / nb:.0f} ticks per block{clock}")
        width = max(len(n) for n in names)
        for i, n in enumerate(names):
            if n != "-" or c[i]:
                print(f"    {n:{width}s} {c[i] / nb:9.0f}  {100 * c[i] / tot:5.1f} %")
        rest = sum(c[len(names):12])
        if rest:
            print(f"    {'(unnamed slots)':{width}s} {rest / nb:9.0f}  {100 * rest / tot:5.1f} %")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kernel", required=True, choices=sorted(KERNELS))
    ap.add_argument("--lib", help="the variant library built by `make variant` with the kernel's timing macro")
    ap.add_argument("--cases", default="", help="substring of the case labels, or an explicit list where the kernel takes one")
    a = ap.parse_args()
    e = KERNELS[a.kernel]
    if not a.lib or not os.path.exists(a.lib):
        sys.exit(f"phase_timing: --lib must name a library built with -D{e['macro']}; build and run it with\n  {make_line(a.kernel)}")
    os.environ["DIFFSEP_LIB_F16" if e["kind"] == "f16" else "DIFFSEP_LIB"] = os.path.abspath(a.lib)
    sys.path.insert(0, os.path.join(ROOT, "diffusion-separation_amd"))
    from diffsep_amd import _lib
    L = _lib.lib(e["kind"])
    if not hasattr(L, e["symbol"]):
        sys.exit(f"phase_timing: {a.lib} has no {e['symbol']}: it was not built with -D{e['macro']}\n  {make_line(a.kernel)}")
    read = getattr(L, e["symbol"])
    read.argtypes, read.restype = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int], ctypes.c_int
    for k, v in e.get("opts", {}).items():
        _lib.check(L.diffsep_set_option(k.encode(), v), L)
    explicit = _explicit(a.cases, 5) is not None
    for label, make in e["cases"](a.cases):
        if a.cases and not explicit and a.cases not in label:
            continue
        us, out = measure(read, make())
        print_table(a.kernel, label, us, out)


if __name__ == "__main__":
    main()
