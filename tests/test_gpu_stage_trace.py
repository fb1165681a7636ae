"""The Python layer over the conv encoder stage issues the launches recorded in tests/golden/stage_trace.json: the same
entries with the same scalar arguments and the same null / non-null pointers, in the same order, for every stage case,
every switch in its non-default state and one eager update and observation gradient of the plain and the FiLM encoder
(tests/golden/gen_stage_trace.py describes the cases and wrote the file). Equal traces mean equal bits and an equal
captured graph, whatever the layer above the kernels looks like."""
import functools
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import gen_stage_trace as gst  # noqa: E402

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _fixture():
    with open(gst.PATH) as f:
        return gst.unpack(json.load(f))


def _check(got, group):
    want = {k: v for k, v in _fixture().items() if k.startswith(group)}
    assert sorted(got) == sorted(want) and want, group
    for name, rows in got.items():
        rows = json.loads(json.dumps(rows))
        for i, (a, b) in enumerate(zip(rows, want[name])):
            assert a == b, f"{name}: launch {i} is {a}, recorded {b}"
        assert len(rows) == len(want[name]), f"{name}: {len(rows)} launches, recorded {len(want[name])}"


def test_stage_cases_launch_as_recorded():
    _check(gst.stage_cases(), "stage/")


def test_switch_cases_launch_as_recorded():
    _check(gst.switch_cases(), "switch/")


@pytest.mark.parametrize("name", gst.UPDATES)
def test_update_and_observation_grad_launch_as_recorded(name):
    _check(gst.update_cases(name), f"update/{name}/")


def test_the_fixture_is_what_the_generator_packs():
    doc = json.load(open(gst.PATH))
    assert gst.pack(gst.unpack(doc)) == doc
    assert len(_fixture()) == len(gst.cm.STAGE_CASES) + 2 * 2 * 2 * len(gst.SWITCHES) + 2 * len(gst.UPDATES)
