"""The convolution dispatch, launch by launch, against the routes recorded before it moved into ds_conv_plan
(tests/golden/conv_routes.json, written by tests/golden/gen_conv_routes.py on the MI355X): for every engine, batch shape and
option set of the fixture, one eager score evaluation must launch the same kernel instantiations with the same profile
classes on the same shapes the same number of times."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("gen_conv_routes", os.path.join(GOLDEN, "gen_conv_routes.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def recorded():
    with open(gen.OUT) as f:
        return json.load(f)


def test_fixture_holds_every_case(recorded):
    want = [cid for tag, _, _ in gen.ENGINES for cid, _, _, _ in gen.cases(tag)]
    assert sorted(recorded["cases"]) == sorted(want) and len(want) == 41
    assert recorded["fields"] == ["kernel"] + list(gen.FIELDS) + ["count"]


@pytest.mark.gpu
@pytest.mark.parametrize("tag", [t for t, _, _ in gen.ENGINES])
def test_routes_match_the_recorded_ones(recorded, tag):
    import torch
    torch.set_grad_enabled(False)
    cus = gen.device_cus()
    assert cus == recorded["cus"], (f"the fixture was recorded on a device with {recorded['cus']} compute units, this one has "
                                    f"{cus}: the tile-count thresholds of the dispatch sit elsewhere, record it again here")
    eng = gen.make_engine(tag)
    try:
        for cid, B, W, opts in gen.cases(tag):
            got = gen.rows(gen.record(eng, B, W, opts))
            want = recorded["cases"][cid]
            if got != want:
                g, w = {tuple(r) for r in got}, {tuple(r) for r in want}
                pytest.fail(f"{cid}: routes differ from the recorded ones\n  only now:      {sorted(g - w)}\n"
                            f"  only recorded: {sorted(w - g)}")
    finally:
        eng.close()
