"""CPU: the parameter layout, buffer sizes, workspace sizes and stage ranges of every handle kind are the recorded ones (tests/golden/layout_pins.json,
made by tests/golden/make_layout_pins.py) -- late fusion {concat, attention, aspect} x ViT and concat x CLIP at 224 / 336, text-only xlmr- and
bert-shaped, image-only at 192 / 224 / 256, each in bf16 and in the parity mode with and without plane pairs.  Nothing is launched."""
import json
import os

import pytest

import smtc_amd  # noqa: F401
import layout_pins as L

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layout_pins.json")) as f:
    PINS = json.load(f)
CASES = L.cases()


def test_every_configuration_is_pinned():
    assert sorted(PINS) == sorted(CASES) and len(CASES) == 30


@pytest.mark.parametrize("cid", sorted(CASES))
def test_layout_and_sizes_are_the_recorded_ones(cid):
    got, want = L.measure(*CASES[cid]), PINS[cid]
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] == want[k], (cid, k)
