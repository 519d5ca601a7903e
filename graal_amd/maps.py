"""Layout maps: the contact matrix in the current genome order, what the contact model expects for that layout, and their residual, as
images computed on the GPU (graal_layout_maps, graal_amd/csrc/maps.h).

    layout_maps(sampler_or_engine, max_px)   -- the three images, the pixel of every sub-fragment and the contigs' pixel ranges (a dict)
    write_maps(folder, prefix, maps)         -- observed.tiff, expected.tiff, residual.tiff (32-bit float TIFF) and map_contigs.tsv

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
