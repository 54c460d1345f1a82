"""The exact scorers and the composed ties.methods give the bits of the build that tests/golden/walk_bits.json records.

The other GPU files hold general weights (alpha and tau outside {0, 1}, arbitrary gsea weights) to error bounds only, which
an addition reordered inside the shared bitmap walk (csrc/bitmap_walk.h) or a changed tie-free column (launch_last_ranks)
would pass.  tools/walk_bits.py runs a fixed table of seeded cases at the seams of the walk -- 65, 4097 and 8193 rows, 17
columns, sets of 1, 2, 63, 64, 65 and g - 1 rows, 9 lists, 65 permutations -- and digests every result; the golden file
holds what it printed on an MI355X for the commit before the walk was shared (cbd959b).  Every case is computed once, here,
and compared: no case is skipped."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "walk_bits.json")) as f:
    GOLDEN = json.load(f)["digests"]
_spec = importlib.util.spec_from_file_location("walk_bits", os.path.join(ROOT, "tools", "walk_bits.py"))
walk_bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(walk_bits)


@pytest.fixture(scope="module")
def table(hip_ctx):
    return dict(walk_bits.cases(hip_ctx))


def test_the_table_is_the_recorded_one(table):
    assert sorted(table) == sorted(GOLDEN)


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_walk_bits(table, name):
    got = walk_bits.digest(table[name]())
    assert got == GOLDEN[name], f"{name}: the result's bytes differ from the recorded build's"
