"""The profiling / A-B tooling cannot drift from the production build: `make variant` (csrc/Makefile) compiles with the production
rule's own flags, into its own directories, and tools/phase_timing.py's table names things that exist.  Dry runs and text
searches only: nothing here compiles."""
import collections
import importlib.util
import os
import re
import shlex
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "diffusion-separation_amd", "csrc")
TOOLS = os.path.join(ROOT, "tools")


def _make_n(*args):
    """the command lines `make -n <args>` would run in csrc/, each as a token list"""
    out = subprocess.run(["make", "-n", "-C", CSRC, "--no-print-directory", *args], check=True, capture_output=True, text=True).stdout
    return [shlex.split(l) for l in out.splitlines() if l.strip()]


def _output(cmd):
    return cmd[cmd.index("-o") + 1] if "-o" in cmd else None


def _compile_of(cmds, obj):
    hits = [c for c in cmds if "-c" in c and _output(c) == obj]
    assert len(hits) == 1, f"{len(hits)} compile lines write {obj}"
    c = hits[0]
    i = c.index("-o")
    return collections.Counter(c[:i] + c[i + 2:])


def _srcs():
    text = open(os.path.join(CSRC, "Makefile")).read()
    return [s[:-4] for s in re.search(r"^SRCS = (.*)$", text, re.M).group(1).split()]


SRCS = _srcs()
PROD_DIR = {"bf16": "build", "f16": "build_f16"}


def test_the_makefile_lists_its_sources():
    assert len(SRCS) >= 20 and "conv3x3_rw" in SRCS and "sde" in SRCS


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("src", SRCS)
def test_variant_compiles_with_the_production_flags(src, kind):
    """The variant's compile line = the production line of the same source and kind + VFLAGS, apart from the output path
    (token multisets: CXXFLAGS, FLAGS_<src> and -DDS_HALF_F16 all have to be there, nothing else)."""
    variant = _compile_of(_make_n("variant", "NAME=t", f"SRC={src}", "VFLAGS=-DX_PROBE=1", f"KIND={kind}"), f"build_variant/t/{src}.o")
    prod = _compile_of(_make_n("-B", f"{PROD_DIR[kind]}/{src}.o"), f"{PROD_DIR[kind]}/{src}.o")
    assert variant == prod + collections.Counter(["-DX_PROBE=1"])
    assert any(t.startswith("--offload-arch=") for t in prod) and "-fno-slp-vectorize" in prod  # (the comparison is not empty-handed)


@pytest.mark.parametrize("kind,lib", [("bf16", "../ab/libdiffsep_hip_t.so"), ("f16", "../ab/libdiffsep_hip_f16_t.so")])
def test_variant_paths(kind, lib):
    """Objects under build_variant/<tag>/, the library under diffusion-separation_amd/ab/, every other object the production
    one of the same kind, nothing under /tmp."""
    cmds = _make_n("variant", "NAME=t", "SRC=conv_mfma norm", "VFLAGS=-DX_PROBE=1", f"KIND={kind}")
    assert not any("/tmp" in t for c in cmds for t in c)
    link = [c for c in cmds if "-shared" in c]
    assert len(link) == 1 and _output(link[0]) == lib
    assert os.path.normpath(os.path.join(CSRC, lib)).startswith(os.path.join(ROOT, "diffusion-separation_amd", "ab") + os.sep)
    objs = [t for t in link[0] if t.endswith(".o")]
    assert sorted(objs) == sorted(f"{'build_variant/t' if s in ('conv_mfma', 'norm') else PROD_DIR[kind]}/{s}.o" for s in SRCS)
    for c in cmds:
        if "-c" in c:
            assert _output(c).startswith(("build_variant/t/", PROD_DIR[kind] + "/"))
    assert {_output(c) for c in cmds if "-c" in c} >= {"build_variant/t/conv_mfma.o", "build_variant/t/norm.o"}


def test_variant_of_rw_rebuilds_rw4():
    """conv3x3_rw4.hip is conv3x3_rw.hip compiled a second time: SRC=conv3x3_rw compiles both with VFLAGS and links both;
    with FROM= (another text for conv3x3_rw alone) conv3x3_rw4 stays the production object."""
    cmds = _make_n("variant", "NAME=t", "SRC=conv3x3_rw", "VFLAGS=-DRW_TIMING")
    for s in ("conv3x3_rw", "conv3x3_rw4"):
        assert _compile_of(cmds, f"build_variant/t/{s}.o")["-DRW_TIMING"] == 1
    link = [c for c in cmds if "-shared" in c][0]
    assert "build_variant/t/conv3x3_rw4.o" in link and "build/conv3x3_rw4.o" not in link and "build/conv3x3_rw.o" not in link
    cmds = _make_n("variant", "NAME=t", "SRC=conv3x3_rw", "VFLAGS=-DRW_TIMING", "FROM=/somewhere/rw_b.hip")
    c = _compile_of(cmds, "build_variant/t/conv3x3_rw.o")
    assert c["/somewhere/rw_b.hip"] == 1 and c["-I."] == 1 and c["conv3x3_rw.hip"] == 0
    link = [c for c in cmds if "-shared" in c][0]
    assert "build/conv3x3_rw4.o" in link and "build_variant/t/conv3x3_rw4.o" not in link


def test_variant_refuses_what_it_cannot_build():
    for args in (["NAME=t"], ["SRC=conv_mfma"], ["NAME=t", "SRC=conv_mfma.hip"], ["NAME=t", "SRC=conv_mfma", "KIND=fp8"],
                 ["NAME=t", "SRC=conv_mfma norm", "FROM=x.hip"]):
        r = subprocess.run(["make", "-n", "-C", CSRC, "variant", *args], capture_output=True, text=True)
        assert r.returncode != 0 and "variant" in r.stderr


def _table():
    spec = importlib.util.spec_from_file_location("phase_timing_tool", os.path.join(TOOLS, "phase_timing.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_driver_imports_without_torch():
    code = "import sys; sys.path.insert(0, sys.argv[1]); import phase_timing; assert 'torch' not in sys.modules; print(len(phase_timing.KERNELS))"
    r = subprocess.run([sys.executable, "-c", code, TOOLS], check=True, capture_output=True, text=True)
    assert int(r.stdout) >= 9


def test_driver_table_names_what_exists():
    mod = _table()
    all_csrc = "".join(open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h")))
    assert {"conv_mfma", "conv3x3_ws", "conv3x3_small", "attn_fused", "stft", "conv3x3_rw", "conv3x3_rw4", "conv3x3_sw", "conv3x3_sws"} <= set(mod.KERNELS)
    for name, e in mod.KERNELS.items():
        path = os.path.join(CSRC, e["source"])
        assert os.path.exists(path), name
        text = open(path).read()
        text += "".join(open(os.path.join(CSRC, h)).read() for h in re.findall(r'#include "([^"]+)"', text))
        assert re.search(r"\b%s\b" % e["macro"], text), f"{name}: {e['macro']} not in {e['source']} or what it includes"
        assert e["source"][:-4] in SRCS and e["kind"] in PROD_DIR
        assert re.search(r"\b%s\b" % e["symbol"], all_csrc), f"{name}: {e['symbol']}"  # (named beside its PT_NAME)
        assert e["rows"] in (1, 2) and len(e["phases"]) == e["rows"]
        assert all(0 < len(p) <= 12 for p in e["phases"]), name
        assert callable(e["cases"])
        assert f"-D{e['macro']}" in mod.make_line(name) and f"SRC={e['source'][:-4]}" in mod.make_line(name)


def test_driver_refuses_to_run_without_a_variant():
    r = subprocess.run([sys.executable, os.path.join(TOOLS, "phase_timing.py"), "--kernel", "conv3x3_sw"], capture_output=True, text=True)
    assert r.returncode != 0 and "variant NAME=" in r.stderr and "-DSW_TIMING" in r.stderr and "KIND=f16" in r.stderr


def test_no_compile_flags_under_tools():
    """csrc/Makefile is the only holder of the library's compile flags: no tool spells out a compile line.  (The stand-alone
    .hip probes say in a comment how to compile THEMSELVES.)"""
    for d, _, files in os.walk(TOOLS):
        for f in files:
            p = os.path.join(d, f)
            try:
                lines = open(p).read().splitlines()
            except UnicodeDecodeError:
                continue
            for i, l in enumerate(lines):
                if "--offload-arch" in l or "-fno-slp-vectorize" in l:
                    assert f.endswith(".hip") and l.lstrip().startswith("//"), f"{os.path.relpath(p, ROOT)}:{i + 1}: {l.strip()}"
