"""The host side's layouts, pinned: every packed-buffer size, every workspace / KV / prefix / suffix size query and every named
workspace offset (with its ld) of the three handles, for the shipped configurations at a fixed list of shapes, must be byte for
byte what tests/golden/host_layout.json records.  The fixture is the output of tools/host_layout_dump.py on a library built from
the commit before the handles' host scaffolding moved into csrc/vqs_host.h (three carvers -- one aligning after a take, two
before -- became one), so it is independent of the code under test.  The size queries touch no device: no GPU needed."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _flat(d, prefix=""):
    for k, v in d.items():
        if isinstance(v, dict):
            yield from _flat(v, f"{prefix}{k}/")
        else:
            yield prefix + k, v


def test_layouts_are_byte_for_byte_the_recorded_ones():
    import host_layout_dump
    with open(os.path.join(ROOT, "tests", "golden", "host_layout.json")) as f:
        want = dict(_flat(json.load(f)))
    got = dict(_flat(json.loads(json.dumps(host_layout_dump.dump()))))
    assert len(want) > 400 and sum(1 for v in want.values() if v == 0) < len(want) // 4      # the fixture is not vacuous
    assert sorted(got) == sorted(want)
    diff = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not diff, diff
