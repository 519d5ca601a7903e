"""graal_block_flips, graal_block_swaps and graal_block_excisions share one set of buffers on the handle (span_moves.h): the layout
records and the 32-byte sub-fragment records (one allocation, written by each call in its own format) are reallocated when (n, S)
changes, the per-span arrays and the hipCUB scratch grow to the largest call of any of them and are then used at a smaller size than
their allocation, by any of them.  Every call on a handle that served other calls must return
exactly what the same call returns as the FIRST call on a fresh handle with the same uploads.  Nothing here is compared with stored
numbers: the other GPU tests tie the fresh-handle results to the restatements; here the restatements only show, before any launch, that
every call used has at least 10 valid spans with a non-zero q, so that a buffer left all zero cannot pass.

The problems are test_score_buffers_gpu's: window_cases.small_cut("w3") under ref_trans_accu (160 bins at n_sub 3 with mixed RF counts:
the flips' mirror pass is live) and small_cut("w1") (240 fragments at n_sub 1, the quirk off), each also in its uncut layout.  The calls:
the largest and the smallest set of flips.tilings(s, None, 3), of swaps.tilings(s, None, 3) and of excise.tilings(s, None, 3) (every
span of both excision sets scores).  At n_sub 1 a flip of one fragment moves
no centre, so problem w1's largest set of flips (every fragment alone) has q = 0 throughout: there "flips_big" is the largest set
that scores, and "flips_all" adds the largest set itself, which is the call the arrays grow to, held to at least 10 valid spans with
contacts in the window instead."""
import numpy as np
import pytest

from graal_amd import excise, flips, swaps
from tests import excise_reference as XR
from tests import flip_reference as FR
from tests import swap_reference as SR
from tests.test_scaffold_gpu import engine_for
from tests.test_score_buffers_gpu import QUIRK, flat, problem

pytestmark = pytest.mark.gpu

# the largest set, the smallest, the largest again, for the three calls: the arrays grow with the first calls, then serve every call at
# smaller and at their full size.  An excision follows a swap and a flip follows an excision at every stage: after the arrays grew, at a
# smaller size, and (UNCUT, and the second test's lists) in another layout and after a change of (n, S)
SEQUENCE = ("flips_big", "swaps_big", "excise_big", "flips_small", "swaps_small", "excise_small", "flips_all", "flips_big", "swaps_big",
            "excise_big", "flips_big")
UNCUT = ("swaps_small", "excise_big", "flips_big", "swaps_big", "excise_small", "flips_small", "flips_all")
MOVES = {"flips": (flips, FR, "flips"), "swaps": (swaps, SR, "swaps"), "excise": (excise, XR, "excisions")}

_SETS, _FRESH = {}, {}


def layout(name, which):
    P, uncut = problem(name)
    return P["S_o_A_frags"] if which == "cut" else uncut


def scoring(name, which, move, frags):
    """On the CPU: how many of the spans are valid with q != 0, and how many valid with contacts != 0."""
    P, _ = problem(name)
    W = MOVES[move][1].window(P, quirk=QUIRK[name])
    q, c, st, _ = getattr(W, MOVES[move][2])(layout(name, which), *frags)
    return int(((st == 0) & (q != 0)).sum()), int(((st == 0) & (c != 0)).sum())


def spans(name, which, call):
    """The fragments of `call` ("flips_big", ...) in the layout: a tuple of int32 arrays."""
    move, size = call.split("_")
    key = (name, which, move)
    if key not in _SETS:
        sets = sorted(MOVES[move][0].tilings(layout(name, which), None, 3), key=lambda x: len(x[0]))
        big = [x for x in sets if scoring(name, which, move, x)[0] >= 10][-1]
        _SETS[key] = {"small": sets[0], "big": big, "all": sets[-1]}
    return _SETS[key][size]


def run(e, call, frags):
    return flat(getattr(e, {"flips": "block_flips_q", "swaps": "block_swaps_q", "excise": "block_excisions_q"}[call.split("_")[0]])(*frags))


def fresh(name, which, call):
    """`call` as the first call on a fresh handle loaded with problem `name` in layout 'cut' or 'uncut' (computed once)."""
    key = (name, which, call)
    if key not in _FRESH:
        P, uncut = problem(name)
        e = engine_for(P, state=uncut if which == "uncut" else None, quirk=QUIRK[name])
        try:
            _FRESH[key] = run(e, call, spans(name, which, call))
        finally:
            e.close()
    return _FRESH[key]


def check(e, name, which, call, step):
    got, want = run(e, call, spans(name, which, call)), fresh(name, which, call)
    assert len(got) == len(want) == 3
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and np.array_equal(g, w), (name, which, call, step, i)


def assert_calls_score(name, which, calls):
    """On the CPU: every call has at least 10 valid spans whose q is not 0 ("flips_all": whose contacts are not 0)."""
    assert FR.VALID == SR.VALID == XR.VALID == 0
    for call in set(calls):
        move, size = call.split("_")
        assert scoring(name, which, move, spans(name, which, call))[1 if size == "all" else 0] >= 10, (name, which, call)


@pytest.mark.parametrize("name", ["w3", "w1"])
def test_reused_handle_equals_fresh_handle(name):
    P, uncut = problem(name)
    assert_calls_score(name, "cut", SEQUENCE)
    assert_calls_score(name, "uncut", UNCUT)
    for move in MOVES:
        assert len(spans(name, "cut", move + "_big")[0]) > len(spans(name, "cut", move + "_small")[0]) > 0
    for which in ("cut", "uncut"):                       # the excisions' sets are the largest and the smallest of the tilings
        assert spans(name, which, "excise_big") is spans(name, which, "excise_all")
    assert len(spans(name, "cut", "flips_all")[0]) >= max(len(spans(name, "cut", move + "_big")[0]) for move in ("flips", "swaps"))
    e = engine_for(P, quirk=QUIRK[name])
    try:
        for step, call in enumerate(SEQUENCE):
            check(e, name, "cut", call, step)
        e.upload_frags(uncut)
        for step, call in enumerate(UNCUT):
            check(e, name, "uncut", call, len(SEQUENCE) + step)
    finally:
        e.close()


def test_another_problem_on_a_used_handle():
    A, _ = problem("w3")
    B, _ = problem("w1")
    assert len(A["S_o_A_frags"]["pos"]) != len(B["S_o_A_frags"]["pos"])
    first = ("swaps_big", "excise_big", "flips_big")
    second = ("flips_all", "swaps_small", "excise_small", "flips_small", "swaps_big", "excise_big", "flips_big")
    assert_calls_score("w3", "cut", first)
    assert_calls_score("w1", "cut", second)
    e = engine_for(A, quirk=True)
    try:
        for step, call in enumerate(first):
            check(e, "w3", "cut", call, step)
        e.upload_subfrags(B["np_sub_frags_id"], B["np_sub_frags_len_bp"], B["np_sub_frags_accu"], B["init_n_sub_frags"],
                          B["mean_squared_frags_per_bin"])
        e.upload_contacts(B["coo_row"], B["coo_col"], B["coo_val"])
        e.set_params(B["param_simu"])
        e.upload_frags(B["S_o_A_frags"])
        e.set_mode(ref_trans_accu=False)
        for step, call in enumerate(second):
            check(e, "w1", "cut", call, len(first) + step)
    finally:
        e.close()
