"""graal_ring_scores at mid-size shapes against the windowed restatement (tests/ring_reference.ring_scores_windowed): contigs over many
64-slot tiles with several waves per x tile, x tiles shared by many short contigs, the window exit on long linear contigs and long
rings, rings shorter than the window, a contact list longer than one grid pass, waves whose contacts span several contigs.
check_shapes() shows on the CPU that the problems reach those shapes: it is a test of its own without a GPU and runs again in front of
every launch.

The problems are window_cases.m1 (25 kb window), m2, and their cut versions with a seeded third of the pieces of at least 2 fragments
turned into rings.  The call sizes its launch from the layout it scores, not from the handle's statistics; m1 and m1_cut run on a
fresh and on a stepped handle all the same (tests/engine_states.py).

Fragments a few bp long lie in these problems, and the reference's ring price of a pair s kb apart is about s^slope times its linear
price: m1's two longest contigs and a few pieces of the cut problems hold a pair whose term is past 2^31 and are RING_NONFINITE in the
restatement and in the engine alike; their values are not compared, their status is."""
import numpy as np
import pytest

from graal_amd.lib import RING_CLOSE, RING_OPEN
from tests import engine_states as ES
from tests import ring_reference as RR
from tests import window_cases as WC
from tests import window_reference as WR

NAMES = ("m1", "m2", "m1_cut", "m2_cut")


def problem(name):
    make = {"m1": lambda: WC.m1(d_max=25.0), "m2": WC.m2, "m1_cut": lambda: RR.with_rings(WC.m1_cut(), 3, seed=3),
            "m2_cut": lambda: RR.with_rings(WC.m2_cut(), 3, seed=4)}[name]
    return ES.cached(("rings-mid", name), make)


def reference(name):
    def run():
        parts = {}
        return RR.ring_scores_windowed(problem(name), parts=parts) + (parts,)
    return ES.cached(("rings-mid-ref", name), run)


def waves_per_tile(lc):
    """rings.h's rule: the waves per 64-slot x tile, from the longest contig of the layout scored."""
    return min(16, max(1, ((int(lc) + 63) // 64 + 7) // 8))


def shapes(name):
    """What the layout and the contact list of a problem engage."""
    P = problem(name)
    s = {k: np.asarray(v, np.int64) for k, v in P["S_o_A_frags"].items()}
    d_max = float(np.float32(P["param_simu"][5]))
    reach = WR.reach_bp(P["param_simu"][5])
    runs = WR._runs(s["id_c"], s["pos"])                                   # label order: the slot order
    lens = np.array([len(m) for _, m in runs])
    base = np.cumsum(lens) - lens
    tile_first, tile_last = base // 64, (base + lens - 1) // 64
    per_tile = np.bincount(tile_first, minlength=int(tile_last.max()) + 1)
    bp = np.array([s["l_cont_bp"][m[0]] for _, m in runs])
    ring = np.array([s["circ"][m[0]] == 1 for _, m in runs])
    window_frags = np.array([int(np.searchsorted(s["start_bp"][m], s["start_bp"][m[0]] + s["len_bp"][m[0]] + reach)) for _, m in runs])
    sid = np.asarray(P["np_sub_frags_id"]).reshape(-1, 4)
    bin_of = np.zeros(int(sid[:, 3].sum()), np.int64)
    for w in range(3):
        bin_of[sid[sid[:, 3] > w, w]] = np.nonzero(sid[:, 3] > w)[0]
    key = s["id_c"][bin_of[np.asarray(P["coo_row"])]]
    pad = (-len(key)) % 64
    waves = np.concatenate([key, np.full(pad, key[-1])]).reshape(-1, 64)
    distinct = 1 + (np.diff(waves, axis=1) != 0).sum(axis=1)
    return {"Sw": waves_per_tile(lens.max()),
            "y_tiles": bool(((lens > 128) & (window_frags > 64)).any()),                  # a wave takes more than one staged y tile
            "shared_tile": bool((per_tile >= 3).any()), "crossing": bool(((tile_last > tile_first) & (lens <= 64)).any()),
            "exit_linear": bool(((bp > reach + 4000) & ~ring).any()), "exit_ring": bool(((bp > reach + 4000) & ring).any()),
            "short_ring": bool((ring & (bp / 1000.0 < d_max) & (lens >= 2)).any()),
            "strides": len(key) > ES.GRID_CONTACTS, "mixed_wave": bool((distinct >= 3).any())}


def check_shapes():
    sh = {name: shapes(name) for name in NAMES}
    assert sh["m1"]["Sw"] == 16 and sh["m2"]["Sw"] == 3 and sh["m1_cut"]["Sw"] == 1 and sh["m2_cut"]["Sw"] == 1
    # a contig over more than one 64-slot y tile, on a single wave (Sw 1) and shared among several (Sw > 1)
    assert sh["m1_cut"]["y_tiles"] and sh["m1"]["y_tiles"] and sh["m2"]["y_tiles"]
    for name in ("m1_cut", "m2_cut"):
        assert sh[name]["shared_tile"] and sh[name]["crossing"] and sh[name]["mixed_wave"] and sh[name]["short_ring"], (name, sh[name])
    assert sh["m1"]["exit_linear"] and sh["m1"]["exit_ring"] and sh["m1_cut"]["exit_linear"] and sh["m1_cut"]["exit_ring"]
    assert sh["m2"]["exit_linear"] and sh["m2_cut"]["exit_ring"]
    assert sh["m1"]["strides"] and sh["m1_cut"]["strides"]
    return sh


def test_problems_reach_their_shapes():
    check_shapes()


def test_every_class_of_terms_counts():
    """Contacts, mass and (on the problems with several sub-fragments per bin) a bin's own pairs each move compared values by more than
    the tolerance: leaving a class out would fail the comparison."""
    for name in NAMES:
        R, C, St, A, parts = reference(name)
        s = problem(name)["S_o_A_frags"]
        heads = np.nonzero((np.asarray(s["pos"]) == 0) & (St <= RING_OPEN))[0]
        tol = 1e-9 * A[heads] + 1
        for cls in ("contact", "mass") + (("own",) if name.startswith("m2") else ()):
            assert (np.abs(parts[cls][heads]) > tol).sum() >= 3, (name, cls)
        assert (St[heads] == RING_CLOSE).any() and (name == "m2" or (St[heads] == RING_OPEN).any())     # (m2 holds no ring)
        assert name == "m2" or (C[heads] > 0).any()
    # the contigs a wave shares with others (Sw > 1) are compared by value too, not only by status
    for name, longest in (("m1", 500), ("m2", 1100)):
        St, s = reference(name)[2], problem(name)["S_o_A_frags"]
        assert ((St <= RING_OPEN) & (np.asarray(s["l_cont"]) >= longest)).any()


@pytest.mark.gpu
@pytest.mark.parametrize("name,state", [("m1", "fresh"), ("m1", "stepped"), ("m2", "fresh"), ("m1_cut", "fresh"), ("m1_cut", "stepped"),
                                        ("m2_cut", "fresh")])
def test_equals_windowed_reference(name, state):
    check_shapes()
    P = problem(name)
    R, C, St, A, _ = reference(name)
    e, layout, _ = ES.engine_in(state, P)
    try:
        q, c, st = e.ring_scores_q()
        q2, c2, st2 = e.ring_scores_q()
    finally:
        e.close()
    scored = St <= RING_OPEN
    print(name, state, int(scored.sum()), "fragments scored: max |q - R|", int(np.max(np.abs(q[scored] - R[scored]))), "max A", int(A.max()))
    assert np.array_equal(st, St) and np.array_equal(c, C)
    assert (q[~scored] == 0).all()
    assert np.all(np.abs(q[scored] - R[scored]) <= 1e-9 * A[scored] + 1)
    assert np.array_equal(q, q2) and np.array_equal(c, c2) and np.array_equal(st, st2)
