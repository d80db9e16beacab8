"""The decimated RSW row (k_row, W > 0) pinned bitwise.

The row pass's loads, exchanges and transforms may be rescheduled, but every
value entering a butterfly and every butterfly's order stay what they were, so
the stepped state and calcN repeat bit for bit.  tests/golden/row_bitwise.json
holds SHA-256 digests recorded with the build before the row's mirror slots
were formed from one load (recorded results only):

* RSW FilteredAB3 1024², 3 steps — the smallest grid on the decimated row
  (W = 2; νtune = 2.5, cfltune = 0.005 as bench.py documents below 2048²);
* RSW FilteredAB3 2048², 2 steps — the compile-time live band KC = 682.

Each from the seeded driver initial condition, with one calcN of that initial
condition.  The same runs with two slabs held by one process take the KC = 0
row (the live band a run-time value) and must give the same digests."""
import hashlib
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "row_bitwise.json")
CASES = {
    "rsw_fab3_1024": dict(n=1024, steps=3, over=dict(nutune=2.5, cfltune=0.005)),
    "rsw_fab3_2048": dict(n=2048, steps=2, over={}),
}


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded(libsw):
    return libsw


def _sha(a):
    return hashlib.sha256(a.tobytes()).hexdigest()


def digests(name, slabs=1):
    """{"ic", "calcN", "state"} digests of case `name` on `slabs` local slabs"""
    from juliaraytracingsw_amd import drivers

    c = CASES[name]
    dec = dict(nranks=slabs, local_slabs=slabs) if slabs > 1 else None
    prob, _ = drivers.rsw_problem(c["n"], "FilteredAB3", decomposition=dec, **c["over"])
    try:
        ic = prob.sol.copy()
        d = {"ic": _sha(ic), "calcN": _sha(prob.calcN(ic))}
        prob.stepforward(c["steps"])
        d["state"] = _sha(prob.sol)
    finally:
        prob.close()
    return d


@pytest.mark.parametrize("slabs", [1, 2])
@pytest.mark.parametrize("name", sorted(CASES))
def test_row_bitwise(name, slabs):
    want = json.load(open(GOLDEN))[name]
    got = digests(name, slabs)
    print(name, slabs, got)
    assert got["ic"] == want["ic"], "the seeded initial condition differs: the digests below do not apply"
    assert got["calcN"] == want["calcN"]
    assert got["state"] == want["state"]
