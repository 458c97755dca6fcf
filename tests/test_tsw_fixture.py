"""tests/golden/tsw_galewsky_p3_ne24.npz is what tests/golden/make_tsw_fixtures.py computes: regenerating it gives the same bytes
(about 25 s with the sparse oracle)."""
import os

import pytest


def test_tsw_fixture_reproduces_bit_for_bit(oracle, golden_dir, tmp_path):
    pytest.importorskip("scipy")
    from tests.golden import make_tsw_fixtures as M
    path = M.build(str(tmp_path))
    with open(path, "rb") as a, open(os.path.join(golden_dir, M.FILE), "rb") as b:
        assert a.read() == b.read()
