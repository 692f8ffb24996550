#!/usr/bin/env python3
"""A/B of library variants (csrc/Makefile, `make variant`) on one stand-alone tool, on one machine, interleaved, two rounds:

    python tools/variant_ab.py --tool "tools/rw_bench.py 20 conv0" "" diffusion-separation_amd/ab/libdiffsep_hip_a.so ...

Each library is a path; "" is the shipped library.  A path whose file name holds "_f16" replaces the half-precision library
(DIFFSEP_LIB_F16), any other the default one (DIFFSEP_LIB); "{lib}" in the tool line becomes the path.  Every child runs under
its own time limit.  The first child that exits non-zero, dies of a signal or runs out of time ends the run with that status:
nothing is started after a fault, an abort or a timeout."""
import argparse
import os
import shlex
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tool", required=True, help='the python tool and its arguments, e.g. "tools/rw_bench.py 20"')
    ap.add_argument("--timeout", type=float, default=120.0, help="seconds per child process (default 120)")
    ap.add_argument("libs", nargs="+", help='variant libraries; "" = the shipped one')
    a = ap.parse_args()
    for p in a.libs:
        if p and not os.path.exists(p):
            sys.exit(f"variant_ab: {p} not found (build it with `make variant`, csrc/Makefile)")
    for rnd in (1, 2):
        for i, p in enumerate(a.libs):
            env = dict(os.environ)
            if p:
                env["DIFFSEP_LIB_F16" if "_f16" in os.path.basename(p) else "DIFFSEP_LIB"] = os.path.abspath(p)
            cmd = [sys.executable] + [w.replace("{lib}", os.path.abspath(p) if p else "") for w in shlex.split(a.tool)]
            print(f"== variant {i}: {p or 'shipped'} (round {rnd})", flush=True)
            try:
                r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.timeout)
                out, rc = r.stdout, r.returncode
            except subprocess.TimeoutExpired as e:  # (run() has killed and reaped the child)
                out, rc = (e.stdout or b"").decode("utf-8", "replace") if isinstance(e.stdout, bytes) else (e.stdout or ""), 124
            sys.stdout.write("".join(l for l in out.splitlines(True) if "amdgpu" not in l))
            if rc != 0:
                what = "ran past its time limit" if rc == 124 else (f"died of signal {-rc}" if rc < 0 else f"exited {rc}")
                print(f"variant_ab: variant {i} ({p or 'shipped'}) {what} in round {rnd}: nothing further is started", flush=True)
                sys.exit(128 - rc if rc < 0 else rc)


if __name__ == "__main__":
    main()
