"""The tile order of the cell kernel (k_cells_tile, csrc/tpg_grid.hip: block id -> tile through tile_of_block, a permutation inside every whole
group of 64 block ids that hands one XCD's blocks 8 adjacent tiles; a last, partial group keeps the identity) against the oracle, bit for bit,
all 20 arrays, Float64 and Float32, through TripolarGrid -- in the product's order (TPG_CELLS_ORDER 1) and in the plain one (0, test library).
A wrong permutation leaves tiles unwritten or written twice, so whole padded arrays are compared.  Tile counts the shapes give:
  4x12: 2, 124x40: 18, 62x30: 10 tiles    no whole group: the identity, whatever the knob;
  3600x1800 as 12-row bands: 120          one whole group and a tail of 56; general and fast rows in one tile, idle waves past the band;
  3602x40: 61 x 6 = 366                   five whole groups that straddle tile rows (61 is no multiple of 8) and a tail of 46.
The references are tests/test_gpu_cells_paired.py's (same shapes: computed once, shared, read-only); the full sizes are tests/test_gpu_grid.py's."""
import os

import numpy as np
import pytest
import torch

from test_gpu_cells_paired import H4, H5, _bits, _build, _id, _reference

pytestmark = pytest.mark.gpu

CASES = [                                                          # the smallest grid first
    ((4, 12, 1), H4, {}, None),
    ((62, 30, 1), H4, {}, None),
    ((124, 40, 1), H4, {}, None),
    ((124, 40, 1), H4, dict(first_pole_longitude=300), None),      # no wave takes the fast path
    ((3602, 40, 1), H4, {}, None),
    ((3600, 1800, 1), H4, {}, (1, 12)),
    ((3600, 1800, 1), H5, {}, (1, 12)),
    ((3600, 1800, 1), H4, {}, (1789, 1800)),
    ((3600, 1800, 1), H5, {}, (1789, 1800)),
]


@pytest.fixture
def order_knob(osg, via_testlib):
    saved = os.environ.get("TPG_CELLS_ORDER")
    yield os.environ
    if saved is None:
        os.environ.pop("TPG_CELLS_ORDER", None)
    else:
        os.environ["TPG_CELLS_ORDER"] = saved
    via_testlib.tpg_reload_config()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("order", [1, 0], ids=["grouped", "plain"])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_both_tile_orders_equal_the_oracle_bit_for_bit(osg, oracle, gpu, order_knob, case, order, dtype):
    ref = _reference(oracle, case, dtype)
    order_knob["TPG_CELLS_ORDER"] = str(order)
    osg._lib.lib().tpg_reload_config()
    g = _build(osg, case, torch.float64 if dtype == np.float64 else torch.float32)
    assert len(ref) == 20
    for name, r in ref.items():
        got = getattr(g, name).cpu().numpy()
        assert got.shape == r.shape and got.dtype == r.dtype, name
        same = _bits(got) == _bits(r)
        assert same.all(), (name, int((~same).sum()), np.argwhere(~same)[:4].tolist())
