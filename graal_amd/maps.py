"""Layout maps: the contact matrix in the current genome order, what the contact model expects for that layout, and their residual, as
images computed on the GPU (graal_layout_maps, graal_amd/csrc/maps.h).

    layout_maps(sampler_or_engine, max_px)   -- the three images, the pixel of every sub-fragment and the contigs' pixel ranges (a dict)
    write_maps(folder, prefix, maps)         -- observed.tiff, expected.tiff, residual.tiff (32-bit float TIFF) and map_contigs.tsv
    window_maps(sampler_or_engine, origins, px_rows, px_cols, bin)   -- chosen windows of the three maps at any bin, down to one
                                                sub-fragment per pixel (graal_map_windows, graal_amd/csrc/map_windows.h; a dict)
    junction_windows(junction_table, soa, sub_id, rank_of_sub, n, px, bin)   -- windows centred on the n weakest junctions
    write_junction_maps(folder, maps, table) -- junction_%03d_{observed,expected,residual}.tiff and map_junctions.tsv

The order is sampler.display_current_matrix's: contigs by ascending label, fragments by position, a fragment's sub-fragments in stored
order, reversed when ori == -1; ``bin`` consecutive sub-fragments of that order share a pixel (image.matrix_image's rule).  The residual
is the Pearson residual (observed - expected) / sqrt(expected) of the Poisson model the engine scores: a misjoin, an inversion or a
misplaced piece shows as a block of large |residual|.
"""
import os

import numpy as np

from . import image
from .junctions import _engine

CONTIG_COLUMNS = ("label", "fragments", "first_pixel", "last_pixel", "head_fragment")
JUNCTION_MAP_COLUMNS = ("junction", "contig", "position", "left_frag", "right_frag", "score", "u0", "bin")


def contig_table(soa, sub_id, pixel_of_sub):
    """One row per contig of layout `soa` in map order (ascending label): its label, its number of fragments, the first and the last pixel
    it touches, and its fragment at position 0 (labels change with every relabel; the head fragment names the contig).  `sub_id` is the
    [n, 4] table of sub-fragment ids (three ids and their count per fragment)."""
    idc = np.asarray(soa["id_c"], dtype=np.int64)
    pos = np.asarray(soa["pos"], dtype=np.int64)
    sid = np.asarray(sub_id, dtype=np.int64).reshape(-1, 4)
    pix = np.asarray(pixel_of_sub, dtype=np.int64)
    n = len(idc)
    big = np.iinfo(np.int64).max
    lo_f = np.full(n, big, dtype=np.int64)
    hi_f = np.full(n, -1, dtype=np.int64)
    for k in range(3):
        has = sid[:n, 3] > k
        p = pix[sid[:n, k][has]]
        ok = p >= 0
        f = np.nonzero(has)[0][ok]
        lo_f[f] = np.minimum(lo_f[f], p[ok])
        hi_f[f] = np.maximum(hi_f[f], p[ok])
    labels, inv, count = np.unique(idc, return_inverse=True, return_counts=True)
    first = np.full(len(labels), big, dtype=np.int64)
    last = np.full(len(labels), -1, dtype=np.int64)
    np.minimum.at(first, inv, lo_f)
    np.maximum.at(last, inv, hi_f)
    first[first == big] = -1
    head = np.full(len(labels), -1, dtype=np.int64)
    h = np.nonzero(pos == 0)[0]
    head[inv[h]] = h
    return {"label": labels, "fragments": count, "first_pixel": first, "last_pixel": last, "head_fragment": head}


def layout_maps(sampler_or_engine, max_px=2048):
    """The maps of the engine's current layout: a dict with observed, expected, residual (float32 [m, m]), pixel_of_sub (int32 per
    sub-fragment id), bin (sub-fragments per pixel), bad_pixels (pixels whose expected value is not finite) and contigs (contig_table)."""
    e = _engine(sampler_or_engine)
    obs, exp, res, pix, b, bad = e.layout_maps(max_px)
    return {"observed": obs, "expected": exp, "residual": res, "pixel_of_sub": pix, "bin": b, "bad_pixels": bad,
            "contigs": contig_table(e.download_frags(), e.sub_id, pix)}


def write_maps(folder, prefix, maps):
    """Write `maps` (layout_maps' dict) into `folder`: <prefix>observed.tiff, <prefix>expected.tiff, <prefix>residual.tiff and
    <prefix>map_contigs.tsv (a header line, then one row per contig: CONTIG_COLUMNS).  Returns the four paths."""
    os.makedirs(folder, exist_ok=True)
    paths = []
    for name in ("observed", "expected", "residual"):
        paths.append(os.path.join(folder, "%s%s.tiff" % (prefix, name)))
        image.write_tiff_f32(paths[-1], maps[name])
    t = maps["contigs"]
    paths.append(os.path.join(folder, "%smap_contigs.tsv" % prefix))
    with open(paths[-1], "w") as fh:
        fh.write("\t".join(CONTIG_COLUMNS) + "\n")
        for i in range(len(t["label"])):
            fh.write("\t".join(str(int(t[c][i])) for c in CONTIG_COLUMNS) + "\n")
    return paths


def rank_of_sub(soa, sub_id):
    """The rank of every sub-fragment id in the genome order of layout `soa` (contigs by ascending label, fragments by position, a
    fragment's sub-fragments in stored order, reversed when ori == -1), on the host: what window_maps returns as rank_of_sub, for
    choosing windows before the call that renders them."""
    sid = np.asarray(sub_id, dtype=np.int64).reshape(-1, 4)
    n = len(np.asarray(soa["id_c"]))
    order = np.lexsort((np.asarray(soa["pos"], dtype=np.int64), np.asarray(soa["id_c"], dtype=np.int64)))
    nsub = sid[:n, 3][order]
    first = np.cumsum(nsub) - nsub
    fwd = np.asarray(soa["ori"], dtype=np.int64)[order] != -1
    rank = np.full(int(sid[:, 3].sum()), -1, dtype=np.int32)
    for k in range(3):
        has = nsub > k
        rank[sid[order[has], k]] = (first + np.where(fwd, k, nsub - 1 - k))[has]
    return rank


def window_maps(sampler_or_engine, origins, px_rows, px_cols=None, bin=1):
    """Windows of the maps of the engine's current layout, all in one call: a dict with observed, expected, residual (float32 [n_win,
    px_rows, px_cols]), origins (int32 [n_win, 2]: the rank of pixel (0, 0)'s first row and column), bin, rank_of_sub (int32 per
    sub-fragment id) and bad_pixels.  Pixel (p, q) of a window covers the row ranks [u0 + p bin, u0 + (p + 1) bin) and the column ranks
    [v0 + q bin, v0 + (q + 1) bin) of the genome order; what lies outside the genome is 0."""
    e = _engine(sampler_or_engine)
    o = np.asarray(origins, dtype=np.int32).reshape(-1, 2)
    obs, exp, res, rank, bad = e.map_windows(o, px_rows, px_cols, bin)
    return {"observed": obs, "expected": exp, "residual": res, "origins": o, "bin": int(bin), "rank_of_sub": rank, "bad_pixels": bad}


def junction_windows(junction_table, soa, sub_id, rank_of_sub, n, px, bin=1):
    """Square windows around the weakest junctions of a layout: the `n` junctions of `junction_table` (junctions.table_from's dict) with
    the lowest finite score, ties by (contig, position), fewer if the table holds fewer.  A junction's window has px x px pixels of `bin`
    ranks and its pixel (px // 2, px // 2) starts at the first rank, in genome order, of the junction's right fragment: the join is the
    upper left corner of the centre pixel.  `soa` is the layout, `sub_id` the [n, 4] table of sub-fragment ids, `rank_of_sub` the rank
    of every sub-fragment id (window_maps, Engine.map_windows).  -> (origins int32 [k, 2], a dict of columns JUNCTION_MAP_COLUMNS)."""
    score = np.asarray(junction_table["score"], dtype=np.float64)
    contig = np.asarray(junction_table["contig"], dtype=np.int64)
    pos = np.asarray(junction_table["position"], dtype=np.int64)
    valid = np.nonzero(np.isfinite(score))[0]
    pick = valid[np.lexsort((pos[valid], contig[valid], score[valid]))][:max(int(n), 0)]
    right = np.asarray(junction_table["right_frag"], dtype=np.int64)[pick]
    sid = np.asarray(sub_id, dtype=np.int64).reshape(-1, 4)
    first = np.where(np.asarray(soa["ori"], dtype=np.int64)[right] == -1, sid[right, np.maximum(sid[right, 3] - 1, 0)], sid[right, 0])
    u0 = np.asarray(rank_of_sub, dtype=np.int64)[first] - (int(px) // 2) * int(bin)
    table = {"junction": pick, "contig": contig[pick], "position": pos[pick],
             "left_frag": np.asarray(junction_table["left_frag"], dtype=np.int64)[pick], "right_frag": right, "score": score[pick],
             "u0": u0, "bin": np.full(len(pick), int(bin), dtype=np.int64)}
    return np.stack([u0, u0], axis=1).astype(np.int32).reshape(-1, 2), table


def write_junction_maps(folder, maps, table):
    """Write the windows `maps` (window_maps' dict) of the junctions `table` (junction_windows' table) into `folder`:
    junction_%03d_observed.tiff, junction_%03d_expected.tiff, junction_%03d_residual.tiff per junction, numbered in the table's order, and
    map_junctions.tsv (a header line, then one row per junction: JUNCTION_MAP_COLUMNS).  Returns the paths."""
    os.makedirs(folder, exist_ok=True)
    paths = []
    k = len(table["junction"])
    for i in range(k):
        for name in ("observed", "expected", "residual"):
            paths.append(os.path.join(folder, "junction_%03d_%s.tiff" % (i, name)))
            image.write_tiff_f32(paths[-1], maps[name][i])
    paths.append(os.path.join(folder, "map_junctions.tsv"))
    with open(paths[-1], "w") as fh:
        fh.write("\t".join(JUNCTION_MAP_COLUMNS) + "\n")
        for i in range(k):
            fh.write("\t".join(repr(float(table[c][i])) if c == "score" else str(int(table[c][i])) for c in JUNCTION_MAP_COLUMNS) + "\n")
    return paths
