"""The nearest-neighbour source index of both oracles (oracle/torch_oracle.py::resize_nearest, oracle/c/vkas_oracle.c::
vko_nearest) against F.interpolate(mode='nearest') itself, on every (in, out) pair with in <= 64 and out <= 128.  CPU only.

torch evaluates min((int)floorf(dst * scale), in - 1) with scale = (float)in / out; the integer form floor(dst * in / out) that
the oracles and the kernel used before differs from it wherever dst * in / out is an integer and the rounded float product
falls just below it (about 2 % of all pairs).  At integer ratios and at the sizes of recipe.RESIZE_CASES the two forms agree,
which is why no committed fixture changed with the formula."""
import numpy as np
import torch
from torch.nn import functional as F

from oracle import c_oracle as C
from oracle import torch_oracle as O
from tests.golden import recipe

N_IN, N_OUT = 64, 128


def torch_index(n_in, n_out):
    """What F.interpolate(mode='nearest') reads: the resize of a float32 index ramp (indices below 2^24 are exact)."""
    ramp = torch.arange(n_in, dtype=torch.float32).view(1, 1, 1, n_in)
    return F.interpolate(ramp, size=(1, n_out), mode='nearest').view(-1).to(torch.int64)


def integer_index(n_in, n_out):
    """The former formula: floor(dst * in / out) in integers."""
    return torch.clamp((torch.arange(n_out, dtype=torch.int64) * n_in) // n_out, max=n_in - 1)


def test_oracles_follow_torch_on_every_pair():
    differ_from_integer = 0
    for n_in in range(1, N_IN + 1):
        ramp64 = torch.arange(n_in, dtype=torch.float64).view(1, 1, 1, n_in)
        for n_out in range(1, N_OUT + 1):
            want = torch_index(n_in, n_out)
            assert torch.equal(O.nearest_axis(n_in, n_out), want), ('torch oracle, index function', n_in, n_out)
            got = O.resize_nearest(ramp64, (1, n_out)).view(-1).to(torch.int64)
            assert torch.equal(got, want), ('torch oracle, x axis', n_in, n_out)
            got_c = torch.from_numpy(C.nearest(ramp64.numpy(), (1, n_out))).view(-1).to(torch.int64)
            assert torch.equal(got_c, want), ('C oracle, x axis', n_in, n_out)
            differ_from_integer += not torch.equal(want, integer_index(n_in, n_out))
    # the scan is not vacuous: the pairs named in the kernel's tests are among those where the two formulas part
    assert differ_from_integer > 50, differ_from_integer
    for pair in ((14, 46), (21, 69), (30, 58), (26, 22)):
        assert not torch.equal(torch_index(*pair), integer_index(*pair)), pair


def test_oracles_follow_torch_on_the_y_axis():
    """The same index function serves both axes: a few pairs, the parting ones among them, on the row axis of both oracles."""
    for n_in, n_out in ((14, 46), (21, 69), (30, 58), (26, 22), (7, 7), (5, 12), (13, 5)):
        col = torch.arange(n_in, dtype=torch.float64).view(1, 1, n_in, 1)
        want = torch_index(n_in, n_out)
        assert torch.equal(O.resize_nearest(col, (n_out, 1)).view(-1).to(torch.int64), want), (n_in, n_out)
        assert torch.equal(torch.from_numpy(C.nearest(col.numpy(), (n_out, 1))).view(-1).to(torch.int64), want), (n_in, n_out)


def test_old_and_new_formula_agree_where_the_fixtures_are():
    """Integer ratios (every resize of the default model: floor halving, the x f heads) and the sizes of recipe.RESIZE_CASES:
    the integer form and torch's float32 form give the same indices, so the committed golden files stand unchanged."""
    for n_in in range(1, 257):
        for f in range(1, 17):
            assert torch.equal(torch_index(n_in, n_in * f), integer_index(n_in, n_in * f)), (n_in, f)
    for m in range(8, 1025):  # a level-0 size and its floor halvings
        for k in (1, 2, 3):
            if m >> k:
                assert torch.equal(torch_index(m >> k, m), integer_index(m >> k, m)), (m, k)
    for hi, wi, ho, wo in recipe.RESIZE_CASES:
        for n_in, n_out in ((hi, ho), (wi, wo)):
            assert torch.equal(torch_index(n_in, n_out), integer_index(n_in, n_out)), (n_in, n_out)
            assert torch.equal(O.nearest_axis(n_in, n_out), integer_index(n_in, n_out)), (n_in, n_out)
    a = recipe.plain_tensor(7, (2, 3, 5, 7))
    assert np.array_equal(C.nearest(a, (12, 20)), F.interpolate(torch.from_numpy(a), size=(12, 20), mode='nearest').numpy())
