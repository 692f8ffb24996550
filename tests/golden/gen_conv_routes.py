"""Record which kernel every launch of one score evaluation goes to: tests/golden/conv_routes.json.

Run on the MI355X at the commit whose routing is the reference (python tests/golden/gen_conv_routes.py).  Only the public
Engine API is used, so the same script runs on any commit; tests/test_conv_route_gpu.py replays the cases through record()
and asserts equality, counts included.

The cases meet every tile-count threshold of the dispatch from both sides on a 256-CU device: at 256 x 64 the register-weight
kernel's 64-cout rule flips between B = 1 and B = 4, at 128 x 32 between B = 4 and B = 16; the streamed-weight kernel's
8-row / 4-row rule and the 128-cout register-weight rule flip between W = 64 and W = 128 one level further down; the
two-launch route of the cat(128, 128) -> 128 blocks needs nf = 128.  The A/B switches ride on the two 16-bit engines at
(16, 64), no_sws on the split engine.
"""
import json
import os
import sys
import time
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "diffusion-separation_amd"),):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "conv_routes.json")
FIELDS = ("cls", "B", "H", "W", "Cin", "Cout", "taps", "skip_cin", "has_res")

# (tag, nf, dtype name in diffsep_amd._lib)
ENGINES = (("nf64_bf16", 64, "BF16"), ("nf64_f16", 64, "F16"), ("nf64_f32", 64, "F32"), ("nf64_split", 64, "F32_SPLIT"),
           ("nf128_bf16", 128, "BF16"))
SHAPES = ((1, 64), (4, 64), (16, 64), (16, 128))  # (B, padded frames W); H = 256 rows by construction
OPTION_SETS = (("no_rw",), ("no_rw128",), ("no_rw_res",), ("no_sw",), ("no_sw_rw",), ("no_sw_rows4",), ("no_wfrag",),
               ("no_attn_fused",), ("rw_small",), ("no_sw", "no_split256"))


def cases(tag):
    """[(case id, B, W, options)] of one engine"""
    out = [(f"{tag}/B{B}_W{W}", B, W, ()) for B, W in SHAPES]
    if tag in ("nf64_bf16", "nf128_bf16"):
        out += [(f"{tag}/B16_W64/" + "+".join(o), 16, 64, o) for o in OPTION_SETS]
    if tag == "nf64_split":
        out.append((f"{tag}/B16_W64/no_sws", 16, 64, ("no_sws",)))
    return out


def make_engine(tag):
    from diffsep_amd import _lib, synth
    from diffsep_amd.engine import Engine, pack_state_dict, param_table
    nf, dtype = next((n, d) for t, n, d in ENGINES if t == tag)
    cfg = _lib.model_config(nf=nf, num_sources=2, dtype=getattr(_lib, dtype))
    sd = synth.synth_state_dict([(n, s) for n, s, _ in param_table(cfg)], 7)
    return Engine(cfg, pack_state_dict(cfg, sd))


def record(eng, B, W, options=()):
    """{(kernel, cls, B, H, W, Cin, Cout, taps, skip_cin, has_res): launches} of one eager score evaluation"""
    import torch
    T = eng.bucket_length(W)
    assert eng.padded_frames(T) == W
    g = torch.Generator().manual_seed(B * 1000 + W)
    xt = torch.randn((B, eng.S, T), generator=g).cuda()
    mix = torch.randn((B, 1, T), generator=g).cuda()
    t = torch.full((B,), 0.5).cuda()
    for o in options:
        eng.set_option(o, 1)
    try:
        eng.profile_begin()
        eng.score(xt, t, mix)
        eng.profile_end()
        recs = eng.profile_records()
    finally:
        for o in options:
            eng.set_option(o, 0)
    return Counter((r["kernel"],) + tuple(int(r[f]) for f in FIELDS) for r in recs)


def rows(counter):
    """the multiset as sorted JSON rows [kernel, cls, ..., has_res, count]"""
    return sorted(list(k) + [n] for k, n in counter.items())


def device_cus():
    import torch
    return int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)


def main():
    import torch
    torch.set_grad_enabled(False)
    out = {"fields": ["kernel"] + list(FIELDS) + ["count"], "cus": device_cus(), "cases": {}}
    for tag, _, _ in ENGINES:
        t0 = time.perf_counter()
        eng = make_engine(tag)
        t1 = time.perf_counter()
        for cid, B, W, opts in cases(tag):
            out["cases"][cid] = rows(record(eng, B, W, opts))
        eng.close()
        print(f"{tag}: engine {t1 - t0:.1f} s, {len(cases(tag))} cases {time.perf_counter() - t1:.1f} s", flush=True)
    with open(OUT, "w") as f:  # one row per line: diffs stay readable
        f.write('{"fields": %s,\n "cus": %d,\n "cases": {\n' % (json.dumps(out["fields"]), out["cus"]))
        body = []
        for cid, rs in out["cases"].items():
            body.append('  %s: [\n%s]' % (json.dumps(cid), ",\n".join("   " + json.dumps(r) for r in rs)))
        f.write(",\n".join(body) + "}}\n")
    json.load(open(OUT))
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {sum(len(v) for v in out['cases'].values())} rows")


if __name__ == "__main__":
    main()
