"""The five native-size entries and their wrappers answer every bad call with the code and the message, character for character, that
tests/golden/native_refusals.json recorded (tests/native_refusals.py says of what and how).  No device."""
import json
import os

from tests import native_refusals

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "native_refusals.json")


def test_native_refusals_are_the_recorded_ones():
    with open(GOLDEN) as f:
        golden = json.load(f)
    got = json.loads(json.dumps(native_refusals.collect()))  # (as JSON holds it: a list for every (code, message) pair)
    assert sorted(got) == sorted(golden)
    for entry in golden:                                     # entry by entry, so that a failure names the one that moved
        assert got[entry] == golden[entry], entry
