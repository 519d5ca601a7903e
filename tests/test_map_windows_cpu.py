"""Map windows without a GPU: the geometry header (graal_amd/csrc/map_window.h, through its host build) against numpy, the choice of the
junction windows (graal_amd.maps.junction_windows) on hand-built tables, and the windows' numpy restatement
(tests/window_map_reference.py) against the layout maps' (tests/map_reference.py) for grid-aligned windows, before it is used on the GPU."""
import ctypes

import numpy as np
import pytest

from graal_amd import image, maps
from tests import map_reference as MR
from tests import util
from tests import window_map_reference as WMR

_i32p = ctypes.POINTER(ctypes.c_int32)


def host_window(S, u0, v0, bin, px_rows, px_cols, p, q, ranks):
    L = util.hostcheck()
    L.hc_map_window.argtypes = [ctypes.c_int] * 6 + [ctypes.c_int, _i32p, _i32p, _i32p, _i32p, _i32p]
    L.hc_map_window.restype = None
    p, q = np.ascontiguousarray(p, dtype=np.int32), np.ascontiguousarray(q, dtype=np.int32)
    ranks = np.ascontiguousarray(ranks, dtype=np.int32)
    out, pix = np.zeros((len(p), 6), dtype=np.int32), np.zeros((len(p), 2), dtype=np.int32)
    L.hc_map_window(S, u0, v0, bin, px_rows, px_cols, len(p), *(x.ctypes.data_as(_i32p) for x in (p, q, ranks, out, pix)))
    return out, pix


#          S,   u0,   v0, bin, px_rows, px_cols
GEOMETRY = [(100, -5, -5, 1, 16, 16),            # negative origins
            (100, 95, 97, 1, 16, 12),            # reaching past S
            (100, 150, 200, 3, 8, 8),            # beyond S
            (100, -400, -300, 7, 8, 9),          # wholly before 0
            (20, -7, -3, 5, 9, 13),              # straddling both ends; bin divides neither the window's start nor S
            (100, 10, 25, 5, 6, 6),              # rows [10, 40) against columns [25, 55): partial overlap
            (100, 30, 30, 4, 5, 5),              # rows and columns the same
            (100, 3, 7, 5, 9, 13),               # pixels overlapping by part of a bin
            (100, 0, 50, 10, 5, 5),              # no overlap
            (2 ** 31 - 1, 2 ** 31 - 50, -2 ** 31, 2 ** 20, 4096, 4096)]   # origin + p bin leaves int32


@pytest.mark.parametrize("S,u0,v0,bin,px_rows,px_cols", GEOMETRY)
def test_host_build_of_the_window_geometry(S, u0, v0, bin, px_rows, px_cols):
    p, q = (x.ravel() for x in np.meshgrid(np.arange(px_rows), np.arange(px_cols), indexing="ij"))
    if len(p) > 4096:
        keep = np.random.RandomState(1).choice(len(p), 4096, replace=False)
        p, q = p[keep], q[keep]
    rng = np.random.RandomState(2)
    ranks = np.stack([np.clip(u0 + rng.randint(-2 * bin, (px_rows + 2) * bin, len(p)), 0, S - 1),
                      np.clip(v0 + rng.randint(-2 * bin, (px_cols + 2) * bin, len(p)), 0, S - 1)], axis=1)
    out, pix = host_window(S, u0, v0, bin, px_rows, px_cols, p, q, ranks)
    clip = lambda x: np.clip(x, 0, S)
    rlo, rhi = clip(u0 + p.astype(np.int64) * bin), clip(u0 + (p.astype(np.int64) + 1) * bin)
    clo, chi = clip(v0 + q.astype(np.int64) * bin), clip(v0 + (q.astype(np.int64) + 1) * bin)
    assert np.array_equal(out[:, 0], rlo) and np.array_equal(out[:, 1], rhi)
    assert np.array_equal(out[:, 2], clo) and np.array_equal(out[:, 3], chi)
    # the overlap, as sets of ranks
    n_both = np.maximum(np.minimum(rhi, chi) - np.maximum(rlo, clo), 0)
    assert np.array_equal(out[:, 5] - out[:, 4], n_both)
    has = n_both > 0
    assert np.array_equal(out[has, 4], np.maximum(rlo, clo)[has]) and np.array_equal(out[has, 5], np.minimum(rhi, chi)[has])
    # the pixel of a rank: the one pixel whose unclipped range holds it, or none
    for side, origin, px in ((0, u0, px_rows), (1, v0, px_cols)):
        d = ranks[:, side].astype(np.int64) - origin
        want = np.where((d >= 0) & (d // bin < px), d // bin, -1)
        assert np.array_equal(pix[:, side], want)
    if S == 100:
        # against explicit sets of ranks
        for i in range(0, len(p), 7):
            R = set(range(u0 + p[i] * bin, u0 + (p[i] + 1) * bin)) & set(range(S))
            C = set(range(v0 + q[i] * bin, v0 + (q[i] + 1) * bin)) & set(range(S))
            assert out[i, 1] - out[i, 0] == len(R) and out[i, 3] - out[i, 2] == len(C) and out[i, 5] - out[i, 4] == len(R & C)
            assert not R or (out[i, 0] == min(R) and out[i, 1] == max(R) + 1)


def test_the_geometry_cases_reach_what_they_are_named_for():
    kinds = set()
    for S, u0, v0, bin, px_rows, px_cols in GEOMETRY[:-1]:
        r0, r1, c0, c1 = u0, u0 + px_rows * bin, v0, v0 + px_cols * bin
        kinds.add("negative" if u0 < 0 else "")
        kinds.add("beyond" if u0 >= S else "")
        kinds.add("both ends" if u0 < 0 and r1 > S else "")
        kinds.add("ragged" if (S - u0) % bin else "")
        both = min(r1, c1) - max(r0, c0)
        kinds.add("full" if (r0, r1) == (c0, c1) else "partial" if both > 0 else "none")
    assert kinds >= {"negative", "beyond", "both ends", "ragged", "full", "partial", "none"}


# ---- junction_windows on hand-built tables

def _layout():
    """Two contigs.  Contig 0: fragments 0, 1, 2 (2 reversed, 3 sub-fragments); contig 1: fragments 3, 4.  Sub-fragment ids in stored
    order: f0: 0, 1; f1: 2; f2: 3, 4, 5; f3: 6; f4: 7, 8."""
    soa = {"id_c": np.array([0, 0, 0, 1, 1]), "pos": np.array([0, 1, 2, 0, 1]), "ori": np.array([1, 1, -1, 1, 1]),
           "next": np.array([1, 2, -1, 4, -1]), "circ": np.zeros(5, dtype=int)}
    sub_id = np.array([[0, 1, 0, 2], [2, 0, 0, 1], [3, 4, 5, 3], [6, 0, 0, 1], [7, 8, 0, 2]])
    return soa, sub_id


def _table(score):
    """The junctions of _layout in contig order: 0|1, 1|2, 3|4."""
    return {"contig": np.array([0, 0, 1]), "position": np.array([0, 1, 0]), "left_frag": np.array([0, 1, 3]),
            "right_frag": np.array([1, 2, 4]), "score": np.array(score, dtype=np.float64)}


def test_rank_of_sub_is_the_reference_order():
    soa, sub_id = _layout()
    rank = maps.rank_of_sub(soa, sub_id)
    assert rank.tolist() == [0, 1, 2, 5, 4, 3, 6, 7, 8]       # (fragment 2 reversed: its ids 3, 4, 5 take ranks 5, 4, 3)
    for name in ("sub3", "sub1", "circ", "wide"):
        P = MR.case(name)
        order = MR.order_of(P["np_sub_frags_id"], P["S_o_A_frags"])
        got = maps.rank_of_sub(P["S_o_A_frags"], P["np_sub_frags_id"])
        assert np.array_equal(got[order], np.arange(len(order))) and (got >= 0).all()


def test_junction_windows_centre_rule_and_clipping():
    soa, sub_id = _layout()
    rank = maps.rank_of_sub(soa, sub_id)
    # the weakest junction is 1|2: fragment 2 is reversed, so its first rank in genome order is that of its LAST stored id (5): rank 3
    origins, t = maps.junction_windows(_table([5.0, -2.0, 1.0]), soa, sub_id, rank, 1, 4, 1)
    assert origins.dtype == np.int32 and origins.tolist() == [[1, 1]] and t["junction"].tolist() == [1]
    assert (t["left_frag"].tolist(), t["right_frag"].tolist(), t["score"].tolist(), t["u0"].tolist(), t["bin"].tolist()) == ([1], [2], [-2.0], [1], [1])
    assert 1 + (4 // 2) * 1 == rank[5] == 3
    # all three, px 7 (odd: the centre pixel is 3), bin 2: the first junction's window starts before rank 0, the last one's ends past S = 9
    origins, t = maps.junction_windows(_table([0.5, 2.0, 1.0]), soa, sub_id, rank, 3, 7, 2)
    assert t["junction"].tolist() == [0, 2, 1] and t["contig"].tolist() == [0, 1, 0] and t["position"].tolist() == [0, 0, 1]
    assert origins[:, 0].tolist() == [2 - 6, 7 - 6, 3 - 6] and np.array_equal(origins[:, 0], origins[:, 1])
    assert origins[0, 0] < 0 and origins[1, 0] + 7 * 2 > 9
    assert set(t) == set(maps.JUNCTION_MAP_COLUMNS)


def test_junction_windows_ties_and_short_tables():
    soa, sub_id = _layout()
    rank = maps.rank_of_sub(soa, sub_id)
    # ties by (contig, position), whatever the table's order
    _, t = maps.junction_windows(_table([1.0, 1.0, 1.0]), soa, sub_id, rank, 2, 4, 1)
    assert t["junction"].tolist() == [0, 1]
    shuffled = {k: v[[2, 1, 0]] for k, v in _table([1.0, 1.0, 1.0]).items()}
    _, t = maps.junction_windows(shuffled, soa, sub_id, rank, 3, 4, 1)
    assert t["junction"].tolist() == [2, 1, 0] and t["contig"].tolist() == [0, 0, 1]
    # n larger than the number of valid junctions; a junction without a score (NaN) is never drawn
    origins, t = maps.junction_windows(_table([np.nan, 3.0, -1.0]), soa, sub_id, rank, 10, 4, 1)
    assert t["junction"].tolist() == [2, 1] and origins.shape == (2, 2)
    origins, t = maps.junction_windows(_table([np.nan] * 3), soa, sub_id, rank, 4, 4, 1)
    assert origins.shape == (0, 2) and all(len(t[c]) == 0 for c in maps.JUNCTION_MAP_COLUMNS)
    origins, t = maps.junction_windows(_table([1.0, 2.0, 3.0]), soa, sub_id, rank, 0, 4, 1)
    assert origins.shape == (0, 2)


def test_write_junction_maps(tmp_path):
    soa, sub_id = _layout()
    origins, t = maps.junction_windows(_table([0.5, 2.0, 1.0]), soa, sub_id, maps.rank_of_sub(soa, sub_id), 2, 4, 1)
    imgs = {k: np.arange(2 * 16, dtype=np.float32).reshape(2, 4, 4) + i for i, k in enumerate(("observed", "expected", "residual"))}
    paths = maps.write_junction_maps(str(tmp_path), imgs, t)
    assert len(paths) == 7
    assert np.array_equal(image.read_tiff_f32(str(tmp_path / "junction_001_expected.tiff")), imgs["expected"][1])
    lines = open(str(tmp_path / "map_junctions.tsv")).read().splitlines()
    assert lines[0].split("\t") == list(maps.JUNCTION_MAP_COLUMNS) and len(lines) == 3
    assert lines[1].split("\t") == ["0", "0", "0", "0", "1", "0.5", str(int(origins[0, 0])), "1"]


# ---- the windows' reference against the layout maps' reference

@pytest.mark.parametrize("name", ["sub3", "sub1", "circ", "wide"])
def test_window_reference_equals_the_map_reference_on_aligned_windows(name):
    """A window whose bin is a layout map's and whose origins are multiples of it is a crop of that map (padded with zeros outside)."""
    S = int(MR.case(name)["init_n_sub_frags"])
    for max_px in MR.MAX_PX[name]:
        R = MR.reference(name, max_px)
        b, m = R["bin"], R["m"]
        pr, pc = min(m, 5) + 2, min(m, 4) + 3
        origins = np.array([[0, 0], [b * (m // 2), 0], [b * (m - 3), b * (m - 2)], [-2 * b, b], [b * m, 0]])
        W = WMR.windows(name, origins, pr, pc, b)
        for w, (u0, v0) in enumerate(origins):
            for key, dtype in (("observed", np.float64), ("expected", np.float64), ("terms", np.int64)):
                want = np.zeros((pr, pc), dtype=dtype)
                p0, q0 = u0 // b, v0 // b
                for p in range(pr):
                    for q in range(pc):
                        if 0 <= p0 + p < m and 0 <= q0 + q < m:
                            want[p, q] = R[key][p0 + p, q0 + q]
                got = W[key][w]
                if key == "expected":
                    assert np.all(np.abs(got - want) <= 1e-12 * want), (max_px, w)
                else:
                    assert np.array_equal(got, want), (max_px, w, key)
        assert W["observed"].sum() > 0 and W["expected"][4].sum() == 0 and S <= b * m


@pytest.mark.parametrize("name", ["sub3", "circ"])
def test_pair_pricing_reference_equals_the_block_sums(name):
    """window_map_reference.windows_of (the mid-size tests' reference: only the window's pairs and contacts) against the block sums of
    the whole bin-1 matrices, misaligned and straddling the diagonal."""
    P = MR.case(name)
    origins = np.array([[3, 7], [-4, 2], [40, 33], [120, 125]])
    A = WMR.windows(name, origins, 9, 13, 5)
    B = WMR.windows_of(P, P["S_o_A_frags"], origins, 9, 13, 5, rows=16)
    assert np.array_equal(A["observed"], B["observed"]) and np.array_equal(A["terms"], B["terms"])
    assert np.all(np.abs(A["expected"] - B["expected"]) <= 1e-12 * A["expected"])
    assert A["terms"].max() == 25 and (A["terms"] == 20).any() and B["cis"].any()      # (20: five ranks shared by rows and columns)
