"""Poison-tier bodies of the earth mover's distance (tests/poison.py): every output element written, the matching in range, canaries
intact, two runs bit-identical, and no state left in LDS from one pair to the next."""
import numpy as np
import torch

from shapegan_amd import evaluation as E
from poison import poisoned
import emd_reference as X
import test_emd as T

EPS = 1e-4
FORMS = (63, 65, 257, 512)


def snapshot(device, P):
    """numpy copies (renew() may scribble over the tensors): matched batch with its matching, matrix, symmetric matrix."""
    A, B, _ = X.case(P)
    a, b = T.tensor(A[:3], device), T.tensor(B[:3], device)
    emd, match = E.earth_movers_distance(a, b, eps=EPS, return_matching=True)
    return (emd.cpu().numpy().copy(), match.cpu().numpy().copy(), E.emd_matrix(a, b, eps=EPS).cpu().numpy().copy(),
            E.emd_matrix(a, a, eps=EPS, symmetric=True).cpu().numpy().copy())


def check_outputs_and_repeat(device, P):
    plain = snapshot(device, P)
    with poisoned() as p:
        first = snapshot(device, P)
        p.renew()
        second = snapshot(device, P)
        p.check_canaries()
    for got in (first, second):
        emd, match, matrix, sym = got
        assert not np.isnan(emd).any() and not np.isnan(matrix).any() and not np.isnan(sym).any(), "P = %d: NaN left" % P
        assert (match >= 0).all() and (match < P).all()
        for s in range(len(match)):
            assert np.array_equal(np.sort(match[s]), np.arange(P))
        for x, y in zip(got, plain):
            np.testing.assert_array_equal(x, y)


def check_raw_outputs(device):
    """sg_emd_match with every optional output: rounds and status are written too."""
    A, B, _ = X.case(65)
    with poisoned() as p:
        emd, match, rounds, status = T.raw_match(A[:4], B[:4], EPS, device)
        p.check_canaries()
    assert not np.isnan(emd).any() and not status.any() and (rounds > 0).all() and (rounds < T.ROUND_CAP).all()
    assert (match >= 0).all() and (match < 65).all()


def check_second_pair_sees_no_state(device):
    """A second, different pair right after a first one: prices, owners, bids and lists of the first are not its start.  Compared
    with the twin's result for the second pair alone (the twin holds no state between pairs: its scratch is rebuilt per pair, and
    its result does not depend on what ran before — asserted by running it in both orders)."""
    A, B, _ = X.case(257)
    alone = T.raw_match(A[1:2], B[2:3], EPS, "cpu")
    T.raw_match(A[0:1], B[0:1], EPS, "cpu")
    again = T.raw_match(A[1:2], B[2:3], EPS, "cpu")
    for x, y in zip(alone, again):
        np.testing.assert_array_equal(x, y)
    T.raw_match(A[0:1], B[0:1], EPS, device)
    after = T.raw_match(A[1:2], B[2:3], EPS, device)
    for x, y in zip(after, alone):
        np.testing.assert_array_equal(x, y)
    # and a smaller pair after a larger one: the tails of the LDS arrays beyond its P hold the larger pair's state
    C, D, _ = X.case(63)
    T.raw_match(A[0:1], B[0:1], EPS, device)
    small = T.raw_match(C[:1], D[:1], EPS, device)
    for x, y in zip(small, T.raw_match(C[:1], D[:1], EPS, "cpu")):
        np.testing.assert_array_equal(x, y)
