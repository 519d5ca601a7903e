"""ctypes binding of ``libgraal_hip.so`` (C ABI: ``include/graal_hip.h``).

This is the whole host<->device boundary of the engine: plain pointers and sizes.  There is no CPU
fallback -- if the library or a HIP device is missing, :class:`Engine` raises.
"""
import ctypes
import os

import numpy as np

from . import build as _build

N_OPS = 13
ABI_VERSION = 7
MODE_REF_TRANS_ACCU, MODE_STRICT = 1, 2
MAX_NEIGHBOURS = 10
Q_SCALE = float(1 << 30)
Q_STEP_FAILED = 1 << 32  # graal_eval_candidates_q: added to the first not-finite flag word by a rank whose step failed (include/graal_hip.h)
Q_NAN = -(1 << 63)      # a candidate's Q sum EXACTLY this (INT64_MIN) stands for NaN: a term was not finite (graal_hip.hip: Q_NAN)


def q_to_float(q, c=None, flags=None):
    """A candidate's value from its two int64 sums (graal_hip.hip: q_value): coarse + fine / 2^30; NaN where the fine sum carries the
    not-finite marker (or `flags` is not zero).  `c` -- zero but for a rare candidate -- holds the finite terms of 2^31 log-likelihood units and more, rounded to
    whole units (kernels3.cu:191-210 adds such terms into its float64 sum like any other: the result must stay finite)."""
    q = np.asarray(q, dtype=np.int64)
    out = q.astype(np.float64) / Q_SCALE
    if c is not None:
        c = np.asarray(c, dtype=np.int64)
        if c.any():
            out = np.where(c != 0, c.astype(np.float64) + out, out)
    bad = q == Q_NAN
    if flags is not None:          # (the device buffer of the RCCL path: flags summed over the ranks)
        flags = np.asarray(flags, dtype=np.int64)
        if len(flags) and int(flags.flat[0]) >= Q_STEP_FAILED:
            raise GraalError("the step failed on some rank (a kernel of the step gave up or a list overflowed): the ranks' sums are not scores")
        bad = bad | (flags != 0)
    if bad.any():
        out = np.where(bad, np.nan, out)
    return out
Q_FULL_BAD = -(1 << 63)  # graal_eval_full_q: q[0] == INT64_MIN exactly flags a non-finite / out-of-range term
FIELDS = ("pos", "id_c", "start_bp", "len_bp", "circ", "id", "prev", "next", "l_cont", "l_cont_bp", "ori", "rep",
          "activ", "id_d")  # struct frag, kernels3.cu:9-24

_i32p = ctypes.POINTER(ctypes.c_int32)
_i64p = ctypes.POINTER(ctypes.c_int64)
_f32p = ctypes.POINTER(ctypes.c_float)
_f64p = ctypes.POINTER(ctypes.c_double)

SYMBOLS = ("graal_abi_version", "graal_create", "graal_destroy", "graal_last_error", "graal_set_params",
           "graal_upload_subfrags", "graal_upload_repeats", "graal_upload_contacts", "graal_upload_contacts_f32", "graal_upload_frags", "graal_download_frags",
           "graal_relabel_contigs", "graal_begin_step", "graal_begin_step_launch", "graal_layout_stats", "graal_eval_full_q", "graal_eval_full_params", "graal_eval_candidates_q",
           "graal_eval_candidates", "graal_exchange_bytes", "graal_attach_exchange", "graal_eval_candidates_x", "graal_exchange_selftest", "graal_detach_exchange", "graal_rccl_unique_id", "graal_attach_rccl", "graal_detach_rccl", "graal_upload_distance_ref", "graal_genome_distance", "graal_apply_move", "graal_set_finisher", "graal_set_mode", "graal_set_timing", "graal_set_scan_path", "graal_last_timing", "graal_scan_times", "graal_strict_times", "graal_time_scan", "graal_last_counters", "graal_take_carry_correction", "graal_upload_own_obs", "graal_explode", "graal_run_counters",
           "graal_simulate_contacts", "graal_simulate_fetch", "graal_junction_scores", "graal_junction_bootstrap", "graal_junction_gaps", "graal_end_links", "graal_end_links_fetch",
           "graal_end_links_best", "graal_end_links_mutual_fetch", "graal_end_links_bootstrap", "graal_end_links_bootstrap_fetch", "graal_edit_layout", "graal_insertions", "graal_insertions_fetch", "graal_block_flips",
           "graal_block_swaps", "graal_block_excisions", "graal_ring_scores", "graal_close_rings",
           "graal_layout_maps", "graal_layout_maps_fetch", "graal_map_windows", "graal_map_windows_fetch",
           "graal_upload_proposal_tables", "graal_step", "graal_step_finish", "graal_steps", "graal_host_np_sum", "graal_host_select_move", "graal_host_neighbours", "graal_host_max_dist_intra")

STEP_DONE, STEP_PAUSED, STEP_FALLBACK, STEP_SELECT = 0, 1, 2, 3
JUNCTION_VALID, JUNCTION_END, JUNCTION_CIRCULAR, JUNCTION_NONFINITE = 0, 1, 2, 3   # graal_junction_scores' status bytes
LINK_VALID, LINK_NONFINITE = 0, 1   # graal_end_links' status bytes
INSERT_VALID, INSERT_NONFINITE = 0, 1   # graal_insertions' status bytes
FLIP_VALID, FLIP_WHOLE, FLIP_CIRCULAR, FLIP_NONFINITE = 0, 1, 2, 3   # graal_block_flips' status bytes
SWAP_VALID, SWAP_CIRCULAR, SWAP_NONFINITE = 0, 1, 2   # graal_block_swaps' status bytes
EXCISE_VALID, EXCISE_WHOLE, EXCISE_CIRCULAR, EXCISE_NONFINITE = 0, 1, 2, 3   # graal_block_excisions' status bytes
RING_CLOSE, RING_OPEN, RING_SINGLE, RING_NONFINITE = 0, 1, 2, 3   # graal_ring_scores' status bytes
RINGEDIT_OK, RINGEDIT_BAD_FRAG, RINGEDIT_CIRCULAR, RINGEDIT_SINGLE, RINGEDIT_TWICE = range(5)   # graal_close_rings' status words
# graal_edit_layout's status words
EDIT_OK, EDIT_BAD_CUT, EDIT_DUP_CUT, EDIT_BAD_END, EDIT_CIRCULAR, EDIT_END_TWICE, EDIT_SAME_CONTIG, EDIT_CYCLE = range(8)
STEPS_ROW = 10   # GRAAL_STEPS_ROW: doubles per step in graal_steps' rows


class StepOut(ctypes.Structure):
    """include/graal_hip.h: graal_step_out"""
    _fields_ = [("stats", ctypes.c_int64 * 8), ("max_id", ctypes.c_int32), ("n_neighbours", ctypes.c_int32),
                ("neighbours", ctypes.c_int32 * 128), ("sample_out", ctypes.c_int32), ("op_sampled", ctypes.c_int32),
                ("id_f_sampled", ctypes.c_int32), ("pad", ctypes.c_int32), ("o", ctypes.c_double),
                ("dist_half_units", ctypes.c_int64), ("scores", ctypes.c_double * (128 * N_OPS)), ("full_likelihood", ctypes.c_double)]


_lib = None


def lib_path():
    return _build.HIP_LIB


def load():
    """Load (never build implicitly on the GPU box: the .so travels with the snapshot) the C-ABI library."""
    global _lib
    if _lib is None:
        path = lib_path()
        if not os.path.exists(path):
            raise RuntimeError("libgraal_hip.so is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        L = ctypes.CDLL(path)
        L.graal_last_error.restype = ctypes.c_char_p
        L.graal_last_error.argtypes = [ctypes.c_void_p]
        L.graal_destroy.restype = None
        L.graal_destroy.argtypes = [ctypes.c_void_p]
        L.graal_create.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
        L.graal_set_params.argtypes = [ctypes.c_void_p, _f32p]
        L.graal_upload_subfrags.argtypes = [ctypes.c_void_p, _i32p, _f32p, _i32p, ctypes.c_int32, ctypes.c_int32,
                                            ctypes.c_float]
        L.graal_upload_repeats.argtypes = [ctypes.c_void_p, _i32p, ctypes.c_int32, _i32p, _i32p, ctypes.c_int32, _f32p]
        L.graal_upload_contacts.argtypes = [ctypes.c_void_p, _i32p, _i32p, _i32p, ctypes.c_int64]
        L.graal_upload_contacts_f32.argtypes = [ctypes.c_void_p, _i32p, _i32p, _f32p, ctypes.c_int64]
        L.graal_upload_frags.argtypes = [ctypes.c_void_p, ctypes.POINTER(_i32p), ctypes.c_int32]
        L.graal_download_frags.argtypes = [ctypes.c_void_p, ctypes.POINTER(_i32p)]
        L.graal_relabel_contigs.argtypes = [ctypes.c_void_p, _i32p]
        L.graal_layout_stats.argtypes = [ctypes.c_void_p, _i64p]
        L.graal_begin_step.argtypes = [ctypes.c_void_p, _i64p, _i32p]
        L.graal_begin_step_launch.argtypes = [ctypes.c_void_p]
        L.graal_eval_full_q.argtypes = [ctypes.c_void_p, _i64p]
        L.graal_eval_full_params.argtypes = [ctypes.c_void_p, _f32p, _i64p, _i32p, _i64p]
        L.graal_eval_candidates_q.argtypes = [ctypes.c_void_p, ctypes.c_int32, _i32p, ctypes.c_int32, ctypes.c_int32,
                                              ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
        L.graal_eval_candidates.argtypes = [ctypes.c_void_p, ctypes.c_int32, _i32p, ctypes.c_int32, ctypes.c_int32, _f64p]
        L.graal_exchange_bytes.argtypes = [ctypes.c_int32, _i64p]
        L.graal_attach_exchange.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
                                            ctypes.c_int64, _i64p]
        L.graal_exchange_selftest.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32]
        L.graal_detach_exchange.argtypes = [ctypes.c_void_p]
        L.graal_rccl_unique_id.argtypes = [ctypes.c_void_p]
        L.graal_attach_rccl.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int32, ctypes.c_int32]
        L.graal_detach_rccl.argtypes = [ctypes.c_void_p]
        L.graal_eval_candidates_x.argtypes = [ctypes.c_void_p, ctypes.c_int32, _i32p, ctypes.c_int32, ctypes.c_int32, _i64p, _i64p]
        L.graal_upload_distance_ref.argtypes = [ctypes.c_void_p, _i32p, _i32p, _i32p, _i32p, ctypes.POINTER(ctypes.c_uint8),
                                                ctypes.c_int32]
        L.graal_genome_distance.argtypes = [ctypes.c_void_p, _i64p]
        L.graal_apply_move.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _i32p]
        L.graal_last_timing.argtypes = [ctypes.c_void_p, _f32p]
        L.graal_last_counters.argtypes = [ctypes.c_void_p, _i64p]
        L.graal_run_counters.argtypes = [ctypes.c_void_p, _i64p]
        L.graal_take_carry_correction.argtypes = [ctypes.c_void_p, _i64p, _i32p]
        L.graal_upload_own_obs.argtypes = [ctypes.c_void_p, _f32p, ctypes.c_int32]
        L.graal_explode.argtypes = [ctypes.c_void_p, _i64p]
        L.graal_simulate_contacts.argtypes = [ctypes.c_void_p, ctypes.c_uint64, _i64p]
        L.graal_simulate_fetch.argtypes = [ctypes.c_void_p, _i32p, _i32p, _i32p, ctypes.c_int64]
        L.graal_junction_scores.argtypes = [ctypes.c_void_p, _i64p, ctypes.POINTER(ctypes.c_uint8)]
        L.graal_junction_bootstrap.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int32, ctypes.c_int64, _i64p,
                                               ctypes.POINTER(ctypes.c_uint8), _i32p, _i64p, _i64p, _i64p, _i64p]
        L.graal_junction_gaps.argtypes = [ctypes.c_void_p, _f32p, ctypes.c_int32, ctypes.c_int64, _i64p, ctypes.POINTER(ctypes.c_uint8),
                                          _i32p, _i64p, _i32p, _i32p, _i64p]
        L.graal_end_links.argtypes = [ctypes.c_void_p, ctypes.c_int32, _i64p]
        L.graal_end_links_fetch.argtypes = [ctypes.c_void_p, _i32p, _i32p, _i64p, _i64p, ctypes.POINTER(ctypes.c_uint8), ctypes.c_int64]
        L.graal_end_links_best.argtypes = [ctypes.c_void_p, ctypes.c_int32, _i32p, _i64p, _i64p]
        L.graal_end_links_mutual_fetch.argtypes = [ctypes.c_void_p, _i32p, _i32p, _i64p, ctypes.c_int64]
        L.graal_end_links_bootstrap.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32,
                                                _i64p]
        L.graal_end_links_bootstrap_fetch.argtypes = [ctypes.c_void_p, _i32p, _i32p, _i64p, _i64p, ctypes.POINTER(ctypes.c_uint8), _i32p, _i32p,
                                                      _i64p, _i64p, _i64p, _i64p, ctypes.c_int64]
        L.graal_edit_layout.argtypes = [ctypes.c_void_p, ctypes.c_int32, _i32p, ctypes.c_int32, _i32p, _i32p, _i32p]
        L.graal_insertions.argtypes = [ctypes.c_void_p, ctypes.c_int32, _i64p]
        L.graal_insertions_fetch.argtypes = [ctypes.c_void_p, _i32p, _i32p, ctypes.POINTER(ctypes.c_uint8), _i64p, _i64p,
                                             ctypes.POINTER(ctypes.c_uint8), ctypes.c_int64]
        L.graal_block_flips.argtypes = [ctypes.c_void_p, ctypes.c_int32, _i32p, _i32p, _i64p, _i64p, ctypes.POINTER(ctypes.c_uint8)]
        L.graal_block_swaps.argtypes = [ctypes.c_void_p, ctypes.c_int32, _i32p, _i32p, _i32p, _i64p, _i64p, ctypes.POINTER(ctypes.c_uint8)]
        L.graal_block_excisions.argtypes = [ctypes.c_void_p, ctypes.c_int32, _i32p, _i32p, _i64p, _i64p, ctypes.POINTER(ctypes.c_uint8)]
        L.graal_ring_scores.argtypes = [ctypes.c_void_p, _i64p, _i64p, ctypes.POINTER(ctypes.c_uint8)]
        L.graal_close_rings.argtypes = [ctypes.c_void_p, ctypes.c_int32, _i32p, _i32p]
        L.graal_layout_maps.argtypes = [ctypes.c_void_p, ctypes.c_int32, _i32p, _i32p, _i64p]
        L.graal_layout_maps_fetch.argtypes = [ctypes.c_void_p, _f32p, _f32p, _f32p, _i32p]
        L.graal_map_windows.argtypes = [ctypes.c_void_p, ctypes.c_int32, _i32p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _i64p]
        L.graal_map_windows_fetch.argtypes = [ctypes.c_void_p, _f32p, _f32p, _f32p, _i32p]
        L.graal_set_timing.argtypes = [ctypes.c_void_p, ctypes.c_int32]
        L.graal_set_scan_path.argtypes = [ctypes.c_void_p, ctypes.c_int32]
        L.graal_set_finisher.argtypes = [ctypes.c_void_p, ctypes.c_int32]
        L.graal_set_mode.argtypes = [ctypes.c_void_p, ctypes.c_int32]
        L.graal_scan_times.argtypes = [ctypes.c_void_p, ctypes.c_int32, _f32p]
        L.graal_strict_times.argtypes = [ctypes.c_void_p, ctypes.c_int32, _f32p]
        L.graal_time_scan.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, _f32p]
        _u8p = ctypes.POINTER(ctypes.c_uint8)
        L.graal_upload_proposal_tables.argtypes = [ctypes.c_void_p, _i32p, _f32p, ctypes.c_int32, ctypes.c_int32, _i32p, ctypes.c_int32,
                                                   _i32p, _i32p, ctypes.c_int32, _u8p, _u8p]
        L.graal_step.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_double, ctypes.c_int32,
                                 ctypes.c_int32, ctypes.POINTER(StepOut)]
        L.graal_step_finish.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_int32, ctypes.POINTER(StepOut)]
        L.graal_steps.argtypes = [ctypes.c_void_p, ctypes.c_void_p, _i32p, ctypes.c_int32, ctypes.c_int32, ctypes.c_double, ctypes.c_int32,
                                  ctypes.c_int32, _f64p, _i32p, ctypes.POINTER(StepOut)]
        L.graal_host_np_sum.restype = ctypes.c_double
        L.graal_host_np_sum.argtypes = [_f64p, ctypes.c_int64]
        L.graal_host_select_move.argtypes = [ctypes.c_void_p, _f64p, ctypes.c_int32, ctypes.c_int32]
        L.graal_host_neighbours.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, _i32p, ctypes.c_int32]
        L.graal_host_max_dist_intra.argtypes = [_f64p, ctypes.c_double, ctypes.c_int32, _f64p, _i32p]
        _lib = L
    return _lib


class GraalError(RuntimeError):
    pass


_mdi_p = (ctypes.c_double * 5)()
_mdi_x = ctypes.c_double(0.0)
_mdi_info = ctypes.c_int32(0)


def host_max_dist_intra(p5, val_inter, f32):
    """include/graal_hip.h: graal_host_max_dist_intra -- (x, MINPACK info).  No device needed."""
    L = load()
    _mdi_p[0], _mdi_p[1], _mdi_p[2], _mdi_p[3], _mdi_p[4] = (float(v) for v in p5)
    rc = L.graal_host_max_dist_intra(_mdi_p, float(val_inter), 1 if f32 else 0, ctypes.byref(_mdi_x), ctypes.byref(_mdi_info))
    if rc != 0:
        raise GraalError("graal_host_max_dist_intra failed (%d)" % rc)
    return _mdi_x.value, int(_mdi_info.value)


def _c(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return a


class Engine:
    """One handle = one GPU.  Thin, typed wrapper; every failure raises :class:`GraalError`."""

    def __init__(self, device=0):
        self._L = load()
        self._h = ctypes.c_void_p()
        rc = self._L.graal_create(int(device), ctypes.byref(self._h))
        if rc != 0:
            msg = self._L.graal_last_error(self._h).decode() if self._h else "graal_create failed"
            if self._h:
                self._L.graal_destroy(self._h)
                self._h = ctypes.c_void_p()
            raise GraalError("graal_create(device=%d): %s" % (device, msg))
        self.device = int(device)
        self.n = 0
        self._x_map = self._x_view = None
        # buffers of the per-step calls, allocated once (numpy's .ctypes accessor costs more than the call itself)
        self._fb_buf = np.zeros(MAX_NEIGHBOURS, dtype=np.int32)
        self._fb_ptr = self._fb_buf.ctypes.data_as(_i32p)
        self._delta_buf = np.zeros(MAX_NEIGHBOURS * N_OPS, dtype=np.float64)
        self._delta_ptr = self._delta_buf.ctypes.data_as(_f64p)
        self._q_buf = np.zeros(MAX_NEIGHBOURS * N_OPS, dtype=np.int64)
        self._q_ptr = self._q_buf.ctypes.data_as(_i64p)
        self._c_buf = np.zeros(MAX_NEIGHBOURS * N_OPS, dtype=np.int64)     # the coarse sums (graal_eval_candidates_x)
        self._c_ptr = self._c_buf.ctypes.data_as(_i64p)
        self._st_buf = np.zeros(8, dtype=np.int64)
        self._st_ptr = self._st_buf.ctypes.data_as(_i64p)
        self._max_id = ctypes.c_int32(0)
        self._max_id_ref = ctypes.byref(self._max_id)

    def close(self):
        if getattr(self, "_h", None):
            self._L.graal_destroy(self._h)   # (unregisters the exchange segment before its mapping goes away)
            self._h = ctypes.c_void_p()
        if getattr(self, "_x_view", None) is not None:
            self._x_view = None
            try:
                self._x_map.close()
            except (BufferError, ValueError):
                pass
            self._x_map = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc, what):
        if rc != 0:
            raise GraalError("%s: %s (code %d)" % (what, self._L.graal_last_error(self._h).decode(), rc))

    # -- uploads ------------------------------------------------------------------------------
    def set_params(self, param8):
        p = _c(np.asarray(param8, dtype=np.float32).reshape(8), np.float32)
        self._ck(self._L.graal_set_params(self._h, p.ctypes.data_as(_f32p)), "graal_set_params")
        self.param = p.copy()   # a host copy of the parameters in force, nothing else changes (graal_amd.flips derives its window from d_max)

    def upload_subfrags(self, sub_id, sub_len_kb, sub_accu, n_sub_total, n_frags_per_bins):
        sid = _c(np.asarray(sub_id).reshape(-1, 4), np.int32)
        sl = _c(np.asarray(sub_len_kb).reshape(-1, 3), np.float32)
        sa = _c(np.asarray(sub_accu).reshape(-1, 3), np.int32)
        assert len(sid) == len(sl) == len(sa)
        self._ck(self._L.graal_upload_subfrags(self._h, sid.ctypes.data_as(_i32p), sl.ctypes.data_as(_f32p),
                                               sa.ctypes.data_as(_i32p), len(sid), int(n_sub_total),
                                               ctypes.c_float(float(n_frags_per_bins))), "graal_upload_subfrags")
        self.n_sub_total = int(n_sub_total)
        self.sub_id = sid.copy()   # a host copy of the id table, nothing else changes (graal_amd.maps names a contig's pixels with it)

    def upload_repeats(self, dup_bins, dispatcher, collector, obs_rows):
        """Repeated bins: their ids, the copies of every bin, and their rows of the observation matrix
        ([n_dup, 3, n_sub_total] float32).  Call between upload_subfrags and upload_contacts / upload_frags."""
        d = _c(dup_bins, np.int32)
        disp = _c(np.asarray(dispatcher).reshape(-1, 2), np.int32)
        coll = _c(collector, np.int32)
        obs = _c(np.asarray(obs_rows, dtype=np.float32).reshape(len(d), 3, -1), np.float32)
        self._ck(self._L.graal_upload_repeats(self._h, d.ctypes.data_as(_i32p), len(d), disp.ctypes.data_as(_i32p),
                                              coll.ctypes.data_as(_i32p), len(coll), obs.ctypes.data_as(_f32p)),
                 "graal_upload_repeats")

    def upload_contacts(self, row, col, count):
        """Counts may be integers or float32 (blacklist fill); integer arrays go through the int32 entry point."""
        r, c = _c(row, np.int32), _c(col, np.int32)
        count = np.asarray(count)
        assert len(r) == len(c) == len(count)
        if np.issubdtype(count.dtype, np.integer):
            v = _c(count, np.int32)
            self._ck(self._L.graal_upload_contacts(self._h, r.ctypes.data_as(_i32p), c.ctypes.data_as(_i32p),
                                                   v.ctypes.data_as(_i32p), len(r)), "graal_upload_contacts")
        else:
            v = _c(count, np.float32)
            self._ck(self._L.graal_upload_contacts_f32(self._h, r.ctypes.data_as(_i32p), c.ctypes.data_as(_i32p),
                                                       v.ctypes.data_as(_f32p), len(r)), "graal_upload_contacts_f32")
        self.nnz = len(r)

    def upload_frags(self, soa):
        arrs = [_c(soa[k], np.int32) for k in FIELDS]
        n = len(arrs[0])
        assert all(len(a) == n for a in arrs)
        ptrs = (_i32p * 14)(*[a.ctypes.data_as(_i32p) for a in arrs])
        self._ck(self._L.graal_upload_frags(self._h, ptrs, n), "graal_upload_frags")
        self.n = n

    def download_frags(self, out=None):
        if out is None:
            out = {k: np.empty(self.n, dtype=np.int32) for k in FIELDS}
        ptrs = (_i32p * 14)(*[out[k].ctypes.data_as(_i32p) for k in FIELDS])
        self._ck(self._L.graal_download_frags(self._h, ptrs), "graal_download_frags")
        return out

    # -- layout maintenance ------------------------------------------------------------------
    def relabel_contigs(self):
        m = ctypes.c_int32(0)
        self._ck(self._L.graal_relabel_contigs(self._h, ctypes.byref(m)), "graal_relabel_contigs")
        return int(m.value)

    def begin_step_launch(self):
        """Launch what begin_step launches and return at once (optional; begin_step then only waits)."""
        self._ck(self._L.graal_begin_step_launch(self._h), "graal_begin_step_launch")

    def begin_step(self):
        """(stats[8], max_id): layout statistics + contig relabel + index rebuild with one synchronisation."""
        rc = self._L.graal_begin_step(self._h, self._st_ptr, self._max_id_ref)
        if rc != 0:
            self._ck(rc, "graal_begin_step")
        return self._st_buf.copy(), int(self._max_id.value)

    def layout_stats(self):
        out = np.zeros(8, dtype=np.int64)
        self._ck(self._L.graal_layout_stats(self._h, out.ctypes.data_as(_i64p)), "graal_layout_stats")
        return out

    def apply_move(self, fA, fB, op, max_id, wait=True):
        """Commit a candidate.  wait=False does not synchronise (the stale-paste count then comes with begin_step)."""
        st = ctypes.c_int32(0)
        self._ck(self._L.graal_apply_move(self._h, int(fA), int(fB), int(op), int(max_id),
                                          ctypes.byref(st) if wait else None), "graal_apply_move")
        return int(st.value)

    # -- likelihood ---------------------------------------------------------------------------
    def eval_full_q(self):
        q = np.zeros(2, dtype=np.int64)
        self._ck(self._L.graal_eval_full_q(self._h, q.ctypes.data_as(_i64p)), "graal_eval_full_q")
        return q

    def eval_full_params(self, param8=None):
        """graal_eval_full_params: (q[2], stats[8], max_id) -- new parameters (kept in force), relabel, full evaluation, one wait."""
        q = np.zeros(2, dtype=np.int64)
        p = None if param8 is None else _c(np.asarray(param8, dtype=np.float32).reshape(8), np.float32)
        rc = self._L.graal_eval_full_params(self._h, None if p is None else p.ctypes.data_as(_f32p), self._st_ptr, self._max_id_ref,
                                            q.ctypes.data_as(_i64p))
        if rc != 0:
            self._ck(rc, "graal_eval_full_params")
        if p is not None:
            self.param = p.copy()
        return q, self._st_buf.copy(), int(self._max_id.value)

    def eval_full(self):
        q = self.eval_full_q()
        if int(q[0]) == Q_FULL_BAD:         # a term was not finite / out of range (the reference would return -inf / NaN)
            return float("nan")
        return float(int(q[0]) + int(q[1])) / Q_SCALE

    def eval_candidates(self, fA, fB, max_id):
        """Delta logL of the 13 candidates of every neighbour: float64 [K, 13].  Single GPU, synchronous."""
        K = len(fB)
        if 1 <= K <= MAX_NEIGHBOURS:   # the per-step path: preallocated buffers, cached pointers (this call is ~10 % of a step)
            self._fb_buf[:K] = fB
            rc = self._L.graal_eval_candidates(self._h, int(fA), self._fb_ptr, K, int(max_id), self._delta_ptr)
            if rc != 0:
                self._ck(rc, "graal_eval_candidates")
            return self._delta_buf[:K * N_OPS].reshape(K, N_OPS).copy()
        fb = _c(fB, np.int32)
        out = np.zeros((len(fb), N_OPS), dtype=np.float64)
        for k0 in range(0, len(fb), MAX_NEIGHBOURS):  # > 10 neighbours (copies of repeated bins): one scan pass per group of 10
            out[k0:k0 + MAX_NEIGHBOURS] = self.eval_candidates(fA, fb[k0:k0 + MAX_NEIGHBOURS], max_id)
        return out

    # -- genome distance ------------------------------------------------------------------------
    def upload_distance_ref(self, init_prev, init_next, init_ori, orientable, counted):
        a = [_c(x, np.int32) for x in (init_prev, init_next, init_ori, orientable)]
        c = _c(counted, np.uint8)
        assert all(len(x) == len(c) for x in a)
        self._ck(self._L.graal_upload_distance_ref(self._h, *[x.ctypes.data_as(_i32p) for x in a],
                                                   c.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), len(c)),
                 "graal_upload_distance_ref")

    def simulate_contacts(self, seed):
        """graal_simulate_contacts + graal_simulate_fetch: contacts drawn from the uploaded layout under the contact model (one Poisson
        count per sub-fragment pair, seeded Philox4x32-10) as the COO list graal_upload_contacts takes -- (row, col, count) int32, row < col,
        sorted by (row, col).  Needs sub-fragments, parameters and fragments, no contacts."""
        nnz = ctypes.c_int64(0)
        self._ck(self._L.graal_simulate_contacts(self._h, ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), ctypes.byref(nnz)),
                 "graal_simulate_contacts")
        n = int(nnz.value)
        row, col, cnt = (np.zeros(n, dtype=np.int32) for _ in range(3))
        self._ck(self._L.graal_simulate_fetch(self._h, row.ctypes.data_as(_i32p), col.ctypes.data_as(_i32p), cnt.ctypes.data_as(_i32p), n),
                 "graal_simulate_fetch")
        return row, col, cnt

    def junction_scores(self):
        """graal_junction_scores: (J float64[n], status uint8[n]), indexed by fragment.  J[f] = logL(layout) - logL(layout cut between f and
        next[f]) in the exact arithmetic, NaN where there is no score; status JUNCTION_VALID / _END / _CIRCULAR / _NONFINITE.  Needs
        sub-fragments, parameters, fragments and contacts; one rank, no repeated bins.  Leaves the step state alone."""
        q, st = self.junction_scores_q()
        return np.where(st == JUNCTION_VALID, q.astype(np.float64) / Q_SCALE, np.nan), st

    def junction_scores_q(self):
        """The same as (int64 Q[n], status uint8[n])."""
        n = int(self.n)
        q = np.zeros(n, dtype=np.int64)
        st = np.zeros(n, dtype=np.uint8)
        self._ck(self._L.graal_junction_scores(self._h, q.ctypes.data_as(_i64p), st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))),
                 "graal_junction_scores")
        return q, st

    def junction_bootstrap(self, seed, n_rep, threshold=0.0, replicates=False):
        """graal_junction_bootstrap as floats: a dict of J (the data's own score), status, support (the fraction of the n_rep Poisson-
        bootstrap replicates of the contacts in which the junction scores above `threshold`, in [0, 1]), mean, min and max of the
        replicate scores, indexed by fragment, NaN where the status is not JUNCTION_VALID; with replicates=True also the matrix
        `replicates` float64[n_rep, n].  Replicate r is a function of (layout, contacts, seed, r) alone.  Same preconditions and refusals
        as junction_scores.  Leaves the step state alone."""
        t = self.junction_bootstrap_q(seed, n_rep, int(round(float(threshold) * Q_SCALE)), replicates)
        ok = t["status"] == JUNCTION_VALID
        out = {"J": np.where(ok, t["q"].astype(np.float64) / Q_SCALE, np.nan), "status": t["status"],
               "support": np.where(ok, t["support"].astype(np.float64) / float(n_rep), np.nan),
               "mean": np.where(ok, t["q_sum"].astype(np.float64) / float(n_rep) / Q_SCALE, np.nan),
               "min": np.where(ok, t["q_min"].astype(np.float64) / Q_SCALE, np.nan),
               "max": np.where(ok, t["q_max"].astype(np.float64) / Q_SCALE, np.nan)}
        if replicates:
            out["replicates"] = np.where(ok[None, :], t["q_rep"].astype(np.float64) / Q_SCALE, np.nan)
        return out

    def junction_bootstrap_q(self, seed, n_rep, threshold_q=0, replicates=False):
        """The same in Q: a dict of q int64[n], status uint8[n], support int32[n] (a count of replicates), q_sum, q_min, q_max int64[n]
        and, with replicates=True, q_rep int64[n_rep, n]; zeros where the status is not JUNCTION_VALID."""
        n, n_rep = int(self.n), int(n_rep)
        q, q_sum, q_min, q_max = (np.zeros(n, dtype=np.int64) for _ in range(4))
        st = np.zeros(n, dtype=np.uint8)
        sup = np.zeros(n, dtype=np.int32)
        rep = np.zeros((max(n_rep, 0), n), dtype=np.int64) if replicates and 1 <= n_rep <= 1024 else None
        self._ck(self._L.graal_junction_bootstrap(self._h, ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), n_rep, int(threshold_q),
                                                  q.ctypes.data_as(_i64p), st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                                  sup.ctypes.data_as(_i32p), q_sum.ctypes.data_as(_i64p), q_min.ctypes.data_as(_i64p),
                                                  q_max.ctypes.data_as(_i64p), rep.ctypes.data_as(_i64p) if rep is not None else None),
                 "graal_junction_bootstrap")
        out = {"q": q, "status": st, "support": sup, "q_sum": q_sum, "q_min": q_min, "q_max": q_max}
        if replicates:
            out["q_rep"] = rep
        return out

    def junction_gaps(self, gap_kb, drop=1.92, profile=False):
        """graal_junction_gaps as floats: the likelihood profile of the gap at every junction over the grid gap_kb (kb; ascending, first
        value >= 0, at most 64 values).  A dict of J (graal_junction_scores' score), status, gap_kb (the grid value with the largest
        G = logL(the layout with that gap behind the fragment) - logL(layout)), gap_score (that G), gap_lo_kb / gap_hi_kb (the smallest
        and largest grid value with G within `drop` log-likelihood units of the largest; 1.92 = chi2_1(0.95) / 2) and the grid indices
        best / lo / hi (int32), indexed by fragment; floats are NaN where the status is not JUNCTION_VALID.  With profile=True also
        `profile` float64[n_gaps, n].  Same preconditions and refusals as junction_scores.  Leaves the step state alone."""
        grid = np.ascontiguousarray(gap_kb, dtype=np.float32).reshape(-1)
        t = self.junction_gaps_q(grid, int(round(float(drop) * Q_SCALE)), profile)
        ok = t["status"] == JUNCTION_VALID
        g64 = grid.astype(np.float64)
        out = {"J": np.where(ok, t["q"].astype(np.float64) / Q_SCALE, np.nan), "status": t["status"],
               "gap_kb": np.where(ok, g64[t["best"]], np.nan), "gap_score": np.where(ok, t["q_best"].astype(np.float64) / Q_SCALE, np.nan),
               "gap_lo_kb": np.where(ok, g64[t["lo"]], np.nan), "gap_hi_kb": np.where(ok, g64[t["hi"]], np.nan),
               "best": t["best"], "lo": t["lo"], "hi": t["hi"]}
        if profile:
            out["profile"] = np.where(ok[None, :], t["q_gap"].astype(np.float64) / Q_SCALE, np.nan)
        return out

    def junction_gaps_q(self, gap_kb, drop_q, profile=False):
        """The same in Q: a dict of q int64[n], status uint8[n], best int32[n] (a grid index), q_best int64[n], lo / hi int32[n] (grid
        indices: the interval with G >= q_best - drop_q) and, with profile=True, q_gap int64[n_gaps, n]; zeros where the status is not
        JUNCTION_VALID."""
        grid = np.ascontiguousarray(gap_kb, dtype=np.float32).reshape(-1)
        n, m = int(self.n), len(grid)
        q, q_best = (np.zeros(n, dtype=np.int64) for _ in range(2))
        st = np.zeros(n, dtype=np.uint8)
        best, lo, hi = (np.zeros(n, dtype=np.int32) for _ in range(3))
        prof = np.zeros((m, n), dtype=np.int64) if profile else None
        self._ck(self._L.graal_junction_gaps(self._h, grid.ctypes.data_as(_f32p), m, int(drop_q), q.ctypes.data_as(_i64p),
                                             st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), best.ctypes.data_as(_i32p),
                                             q_best.ctypes.data_as(_i64p), lo.ctypes.data_as(_i32p), hi.ctypes.data_as(_i32p),
                                             prof.ctypes.data_as(_i64p) if prof is not None else None),
                 "graal_junction_gaps")
        out = {"q": q, "status": st, "best": best, "q_best": q_best, "lo": lo, "hi": hi}
        if profile:
            out["q_gap"] = prof
        return out

    def end_links(self, min_frags=1):
        """graal_end_links: the pairs of contig ends the contacts support, as numpy columns (end_a int32, end_b int32, score float64,
        contacts int64, status uint8), sorted by (end_a, end_b).  end = 2 * fragment + side (0: the contig's head, 1: its tail);
        score = logL(the canonical join of the two ends) - logL(layout) in the exact arithmetic, NaN unless status is LINK_VALID.
        Both contigs linear with >= min_frags fragments.  Needs sub-fragments, parameters, fragments and contacts; one rank, no
        repeated bins.  Leaves the step state alone."""
        a, b, q, c, st = self.end_links_q(min_frags)
        return a, b, np.where(st == LINK_VALID, q.astype(np.float64) / Q_SCALE, np.nan), c, st

    def end_links_q(self, min_frags=1):
        """The same with the score as int64 Q: (end_a, end_b, q, contacts, status)."""
        m = ctypes.c_int64(0)
        self._ck(self._L.graal_end_links(self._h, int(min_frags), ctypes.byref(m)), "graal_end_links")
        m = int(m.value)
        a = np.zeros(m, dtype=np.int32)
        b = np.zeros(m, dtype=np.int32)
        q = np.zeros(m, dtype=np.int64)
        c = np.zeros(m, dtype=np.int64)
        st = np.zeros(m, dtype=np.uint8)
        self._ck(self._L.graal_end_links_fetch(self._h, a.ctypes.data_as(_i32p), b.ctypes.data_as(_i32p), q.ctypes.data_as(_i64p),
                                               c.ctypes.data_as(_i64p), st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), m),
                 "graal_end_links_fetch")
        return a, b, q, c, st

    def end_links_best(self, min_frags=1):
        """graal_end_links_best: every end's best partner, and the mutual-best links, without copying the link table out.
        Returns (best_end int32[2n], best_q int64[2n], mutual) indexed by end = 2 * fragment + side; best_end -1 (and best_q 0) where an
        end has no valid link.  mutual = (end_a int32, end_b int32, q int64), sorted by (end_a, end_b): the links whose ends are each
        other's best partner with Q > 0.  Scores in Q (divide by Q_SCALE).  Same preconditions and refusals as end_links."""
        n2 = 2 * int(self.n)
        be = np.zeros(n2, dtype=np.int32)
        bq = np.zeros(n2, dtype=np.int64)
        m = ctypes.c_int64(0)
        self._ck(self._L.graal_end_links_best(self._h, int(min_frags), be.ctypes.data_as(_i32p), bq.ctypes.data_as(_i64p), ctypes.byref(m)),
                 "graal_end_links_best")
        m = int(m.value)
        a = np.zeros(m, dtype=np.int32)
        b = np.zeros(m, dtype=np.int32)
        q = np.zeros(m, dtype=np.int64)
        self._ck(self._L.graal_end_links_mutual_fetch(self._h, a.ctypes.data_as(_i32p), b.ctypes.data_as(_i32p), q.ctypes.data_as(_i64p), m),
                 "graal_end_links_mutual_fetch")
        return be, bq, (a, b, q)

    def end_links_bootstrap(self, seed, n_rep, min_frags=1, threshold=0.0, replicates=False):
        """graal_end_links_bootstrap as floats: a dict of end_a, end_b, contacts and status (end_links' columns, word for word), score
        (the data's own), support (the fraction of the n_rep Poisson-bootstrap replicates of the contacts in which the link scores above
        `threshold`), mutual (the fraction in which it also is the join both of its ends choose: each the other's best partner, ties to
        the lower partner end), mean, min and max of the replicate scores; floats are NaN where the status is not LINK_VALID.  With
        replicates=True also `replicates` float64[n_rep, n_links].  Replicate r is a function of (layout, contacts, seed, r) alone, and
        the same resampled dataset as junction_bootstrap's replicate r under the same seed.  Same preconditions and refusals as
        end_links.  Leaves the step state alone."""
        t = self.end_links_bootstrap_q(seed, n_rep, min_frags, int(round(float(threshold) * Q_SCALE)), replicates)
        ok = t["status"] == LINK_VALID
        f = lambda x, d=1.0: np.where(ok, x.astype(np.float64) / d, np.nan)
        out = {"end_a": t["end_a"], "end_b": t["end_b"], "contacts": t["contacts"], "status": t["status"], "score": f(t["q"], Q_SCALE),
               "support": f(t["support"], float(n_rep)), "mutual": f(t["mutual"], float(n_rep)),
               "mean": f(t["q_sum"], float(n_rep) * Q_SCALE), "min": f(t["q_min"], Q_SCALE), "max": f(t["q_max"], Q_SCALE)}
        if replicates:
            out["replicates"] = np.where(ok[None, :], t["q_rep"].astype(np.float64) / Q_SCALE, np.nan)
        return out

    def end_links_bootstrap_q(self, seed, n_rep, min_frags=1, threshold_q=0, replicates=False):
        """The same in Q: a dict of end_a, end_b int32, q, contacts int64, status uint8, support, mutual int32 (counts of replicates),
        q_sum, q_min, q_max int64 and, with replicates=True, q_rep int64[n_rep, n_links]; replicate columns are 0 where the status is
        not LINK_VALID."""
        m = ctypes.c_int64(0)
        n_rep = int(n_rep)
        self._ck(self._L.graal_end_links_bootstrap(self._h, int(min_frags), ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), n_rep,
                                                   int(threshold_q), 1 if replicates else 0, ctypes.byref(m)), "graal_end_links_bootstrap")
        m = int(m.value)
        a, b, sup, mut = (np.zeros(m, dtype=np.int32) for _ in range(4))
        q, c, q_sum, q_min, q_max = (np.zeros(m, dtype=np.int64) for _ in range(5))
        st = np.zeros(m, dtype=np.uint8)
        rep = np.zeros((n_rep, m), dtype=np.int64) if replicates else None
        self._ck(self._L.graal_end_links_bootstrap_fetch(self._h, a.ctypes.data_as(_i32p), b.ctypes.data_as(_i32p), q.ctypes.data_as(_i64p),
                                                         c.ctypes.data_as(_i64p), st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                                         sup.ctypes.data_as(_i32p), mut.ctypes.data_as(_i32p), q_sum.ctypes.data_as(_i64p),
                                                         q_min.ctypes.data_as(_i64p), q_max.ctypes.data_as(_i64p),
                                                         rep.ctypes.data_as(_i64p) if rep is not None else None, m),
                 "graal_end_links_bootstrap_fetch")
        out = {"end_a": a, "end_b": b, "q": q, "contacts": c, "status": st, "support": sup, "mutual": mut, "q_sum": q_sum, "q_min": q_min,
               "q_max": q_max}
        if replicates:
            out["q_rep"] = rep
        return out

    def insertions(self, max_piece_frags=1):
        """graal_insertions: every insertion of a piece (a linear contig of 1 .. max_piece_frags fragments) into a junction of another
        linear contig that the contacts support, as numpy columns (piece int32, after int32, rev uint8, score float64, contacts int64,
        status uint8), sorted by (after, piece, rev).  piece = the piece's position-0 fragment, after = f: the piece goes between f and
        next[f], its head next to f (rev 0) or its tail (rev 1); score = logL(inserted layout) - logL(layout) in the exact arithmetic,
        NaN unless status is INSERT_VALID.  Same preconditions and refusals as end_links; leaves the step state alone."""
        p, f, r, q, c, st = self.insertions_q(max_piece_frags)
        return p, f, r, np.where(st == INSERT_VALID, q.astype(np.float64) / Q_SCALE, np.nan), c, st

    def insertions_q(self, max_piece_frags=1):
        """The same with the score as int64 Q: (piece, after, rev, q, contacts, status)."""
        m = ctypes.c_int64(0)
        self._ck(self._L.graal_insertions(self._h, int(max_piece_frags), ctypes.byref(m)), "graal_insertions")
        m = int(m.value)
        p = np.zeros(m, dtype=np.int32)
        f = np.zeros(m, dtype=np.int32)
        r = np.zeros(m, dtype=np.uint8)
        q = np.zeros(m, dtype=np.int64)
        c = np.zeros(m, dtype=np.int64)
        st = np.zeros(m, dtype=np.uint8)
        u8 = ctypes.POINTER(ctypes.c_uint8)
        self._ck(self._L.graal_insertions_fetch(self._h, p.ctypes.data_as(_i32p), f.ctypes.data_as(_i32p), r.ctypes.data_as(u8),
                                                q.ctypes.data_as(_i64p), c.ctypes.data_as(_i64p), st.ctypes.data_as(u8), m),
                 "graal_insertions_fetch")
        return p, f, r, q, c, st

    def block_flips(self, first, last):
        """graal_block_flips: for the disjoint blocks (first[k] .. last[k], two fragments of one contig in position order) the score
        F = logL(layout with the block reversed in place) - logL(layout) in the exact arithmetic, as (F float64, contacts int64, status
        uint8) in the caller's order; F is NaN unless status is FLIP_VALID (FLIP_WHOLE: the block is its whole contig, FLIP_CIRCULAR: it
        lies in a ring, FLIP_NONFINITE).  contacts = the summed count between the block and the rest of its contig inside the window of
        the flipped layout.  Same preconditions and refusals as junction_scores; blocks that overlap, span two contigs, run backwards or
        name no fragment raise GraalError.  Leaves the step state alone."""
        q, c, st = self.block_flips_q(first, last)
        return np.where(st == FLIP_VALID, q.astype(np.float64) / Q_SCALE, np.nan), c, st

    def block_flips_q(self, first, last):
        """The same with the score as int64 Q: (q, contacts, status)."""
        first = np.ascontiguousarray(first, dtype=np.int32).reshape(-1)
        last = np.ascontiguousarray(last, dtype=np.int32).reshape(-1)
        if len(first) != len(last):
            raise ValueError("first and last must have the same length")
        m = len(first)
        q = np.zeros(m, dtype=np.int64)
        c = np.zeros(m, dtype=np.int64)
        st = np.zeros(m, dtype=np.uint8)
        self._ck(self._L.graal_block_flips(self._h, m, first.ctypes.data_as(_i32p), last.ctypes.data_as(_i32p), q.ctypes.data_as(_i64p),
                                           c.ctypes.data_as(_i64p), st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))),
                 "graal_block_flips")
        return q, c, st

    def block_swaps(self, first, mid, last):
        """graal_block_swaps: for the disjoint spans (first[k] .. last[k]) of two adjacent runs X = first[k] .. mid[k] and Y = the
        fragments behind mid[k] up to last[k] (three fragments of one contig in position order, mid before last) the score
        S = logL(layout with Y in front of X) - logL(layout) in the exact arithmetic, as (S float64, contacts int64, status uint8) in the
        caller's order; S is NaN unless status is SWAP_VALID (SWAP_CIRCULAR: the runs lie in a ring, SWAP_NONFINITE).  contacts = the
        summed count among the changed pairs inside the window of the swapped layout.  Same preconditions and refusals as
        junction_scores; spans that overlap, span two contigs, come in a wrong order or name no fragment raise GraalError.  Leaves the
        step state alone."""
        q, c, st = self.block_swaps_q(first, mid, last)
        return np.where(st == SWAP_VALID, q.astype(np.float64) / Q_SCALE, np.nan), c, st

    def block_swaps_q(self, first, mid, last):
        """The same with the score as int64 Q: (q, contacts, status)."""
        first = np.ascontiguousarray(first, dtype=np.int32).reshape(-1)
        mid = np.ascontiguousarray(mid, dtype=np.int32).reshape(-1)
        last = np.ascontiguousarray(last, dtype=np.int32).reshape(-1)
        if not len(first) == len(mid) == len(last):
            raise ValueError("first, mid and last must have the same length")
        m = len(first)
        q = np.zeros(m, dtype=np.int64)
        c = np.zeros(m, dtype=np.int64)
        st = np.zeros(m, dtype=np.uint8)
        self._ck(self._L.graal_block_swaps(self._h, m, first.ctypes.data_as(_i32p), mid.ctypes.data_as(_i32p), last.ctypes.data_as(_i32p),
                                           q.ctypes.data_as(_i64p), c.ctypes.data_as(_i64p), st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))),
                 "graal_block_swaps")
        return q, c, st

    def block_excisions(self, first, last):
        """graal_block_excisions: for the disjoint spans (first[k] .. last[k], two fragments of one contig in position order) the score
        E = logL(layout with the span cut out of its contig, the gap closed behind it and the span a contig of its own) - logL(layout)
        in the exact arithmetic, as (E float64, contacts int64, status uint8) in the caller's order; E is NaN unless status is
        EXCISE_VALID (EXCISE_WHOLE: the span is its whole contig, EXCISE_CIRCULAR: it lies in a ring, EXCISE_NONFINITE).  contacts = the
        summed count between the span and the rest of its contig inside the window of the current layout: what the cut severs.  Same
        preconditions and refusals as junction_scores; spans that overlap, span two contigs, run backwards or name no fragment raise
        GraalError.  Leaves the step state alone."""
        q, c, st = self.block_excisions_q(first, last)
        return np.where(st == EXCISE_VALID, q.astype(np.float64) / Q_SCALE, np.nan), c, st

    def block_excisions_q(self, first, last):
        """The same with the score as int64 Q: (q, contacts, status)."""
        first = np.ascontiguousarray(first, dtype=np.int32).reshape(-1)
        last = np.ascontiguousarray(last, dtype=np.int32).reshape(-1)
        if len(first) != len(last):
            raise ValueError("first and last must have the same length")
        m = len(first)
        q = np.zeros(m, dtype=np.int64)
        c = np.zeros(m, dtype=np.int64)
        st = np.zeros(m, dtype=np.uint8)
        self._ck(self._L.graal_block_excisions(self._h, m, first.ctypes.data_as(_i32p), last.ctypes.data_as(_i32p), q.ctypes.data_as(_i64p),
                                               c.ctypes.data_as(_i64p), st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))),
                 "graal_block_excisions")
        return q, c, st

    def ring_scores(self):
        """graal_ring_scores: (R float64[n], contacts int64[n], status uint8[n]), indexed by fragment, every fragment carrying its
        contig's values.  R = logL(layout with the contig in the other topology, every coordinate kept) - logL(layout) in the exact
        arithmetic: closing a linear contig of >= 2 fragments (RING_CLOSE), opening a ring at its wrap (RING_OPEN); NaN for RING_SINGLE
        and RING_NONFINITE.  contacts = the summed count of the contig's contacts closer across the wrap than along the contig (s <
        d_max and 2 s > s_tot).  The ring price is the reference's: only pairs less than d_max apart along the contig change.  Same
        preconditions and refusals as junction_scores.  Leaves the step state alone."""
        q, c, st = self.ring_scores_q()
        return np.where(st <= RING_OPEN, q.astype(np.float64) / Q_SCALE, np.nan), c, st

    def ring_scores_q(self):
        """The same with the score as int64 Q: (q, contacts, status)."""
        n = int(self.n)
        q = np.zeros(n, dtype=np.int64)
        c = np.zeros(n, dtype=np.int64)
        st = np.zeros(n, dtype=np.uint8)
        self._ck(self._L.graal_ring_scores(self._h, q.ctypes.data_as(_i64p), c.ctypes.data_as(_i64p),
                                           st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))), "graal_ring_scores")
        return q, c, st

    def close_rings(self, frags):
        """graal_close_rings: every contig named by one of its fragments in `frags` (linear, >= 2 fragments, named once) becomes a ring:
        circ = 1, the head's prev = the tail, the tail's next = the head, every other field kept.  Returns the status array (int32,
        RINGEDIT_OK everywhere).  A refusal raises GraalError (layout unchanged) with the status array as its .status attribute.
        Afterwards the engine is as after edit_layout.  A ring is opened by edit_layout: a cut after its last-position fragment."""
        f = _c(np.asarray(frags, dtype=np.int64).reshape(-1), np.int32)
        st = np.zeros(len(f), dtype=np.int32)
        rc = self._L.graal_close_rings(self._h, len(f), f.ctypes.data_as(_i32p), st.ctypes.data_as(_i32p))
        if rc != 0:
            try:
                self._ck(rc, "graal_close_rings")
            except GraalError as err:
                err.status, err.code = st, rc
                raise
        return st

    def layout_maps(self, max_px=2048):
        """graal_layout_maps + graal_layout_maps_fetch: (observed, expected, residual, pixel_of_sub, bin, bad_pixels).  The three images
        are float32 [m, m] in the current genome order (contigs by ascending label, fragments by position, sub-fragments in stored order,
        reversed when ori == -1), `bin` consecutive sub-fragments of that order per pixel (bin = max(1, ceil(S / max_px)), 1 <= max_px <=
        4096): the summed contacts between two pixels, what the contact model expects there, and the Pearson residual (observed - expected)
        / sqrt(expected).  pixel_of_sub int32[S]: the pixel of every sub-fragment id.  bad_pixels: pixels whose expected value is not
        finite (NaN in expected and residual).  Same preconditions and refusals as junction_scores.  Leaves the step state alone."""
        m, b = self.layout_maps_compute(max_px)
        obs, exp, res = (np.zeros((m, m), dtype=np.float32) for _ in range(3))
        pix = self.layout_maps_fetch(obs, exp, res)
        return obs, exp, res, pix, b, self._maps_bad

    def layout_maps_compute(self, max_px=2048):
        """graal_layout_maps alone: the images stay on the device; (m, bin)."""
        m, b, bad = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int64(0)
        self._ck(self._L.graal_layout_maps(self._h, int(max_px), ctypes.byref(m), ctypes.byref(b), ctypes.byref(bad)), "graal_layout_maps")
        self._maps_bad = int(bad.value)
        self._maps_m = int(m.value)
        return int(m.value), int(b.value)

    def layout_maps_fetch(self, observed=None, expected=None, residual=None, pixel_of_sub=True):
        """graal_layout_maps_fetch into the given float32 [m, m] arrays (None: not copied); returns pixel_of_sub (or None)."""
        pix = np.zeros(int(getattr(self, "n_sub_total", 0)), dtype=np.int32) if pixel_of_sub else None
        ptr = []
        for a in (observed, expected, residual):
            if a is not None and not (a.dtype == np.float32 and a.flags["C_CONTIGUOUS"] and a.shape == (getattr(self, "_maps_m", -1),) * 2):
                raise ValueError("layout_maps_fetch takes C-contiguous float32 [m, m] arrays of the last layout_maps_compute")
            ptr.append(None if a is None else a.ctypes.data_as(_f32p))
        self._ck(self._L.graal_layout_maps_fetch(self._h, ptr[0], ptr[1], ptr[2], None if pix is None else pix.ctypes.data_as(_i32p)),
                 "graal_layout_maps_fetch")
        return pix

    def map_windows(self, origins, px_rows, px_cols=None, bin=1):
        """graal_map_windows + graal_map_windows_fetch: (observed, expected, residual, rank_of_sub, bad_pixels).  `origins` is [n_win, 2]
        (u0, v0) in ranks of the genome order of layout_maps; the three images are float32 [n_win, px_rows, px_cols] (px_cols defaults to
        px_rows): pixel (p, q) of a window sums the bin-1 maps over the row ranks [u0 + p bin, u0 + (p + 1) bin) and the column ranks
        [v0 + q bin, v0 + (q + 1) bin), cut to the genome; a pixel outside it is 0.  rank_of_sub int32[S]: the rank of every sub-fragment
        id (-1: not ranked).  bad_pixels: pixels whose expected value is not finite (NaN in expected and residual).  Same preconditions
        and refusals as layout_maps; its own buffers.  Leaves the step state alone."""
        shape = self.map_windows_compute(origins, px_rows, px_cols, bin)
        obs, exp, res = (np.zeros(shape, dtype=np.float32) for _ in range(3))
        rank = self.map_windows_fetch(obs, exp, res)
        return obs, exp, res, rank, self._windows_bad

    def map_windows_compute(self, origins, px_rows, px_cols=None, bin=1):
        """graal_map_windows alone: the images stay on the device; their shape (n_win, px_rows, px_cols)."""
        o = np.ascontiguousarray(np.asarray(origins, dtype=np.int32).reshape(-1, 2))
        pc = int(px_rows if px_cols is None else px_cols)
        bad = ctypes.c_int64(0)
        self._windows_shape = None
        self._ck(self._L.graal_map_windows(self._h, len(o), o.ctypes.data_as(_i32p), int(px_rows), pc, int(bin), ctypes.byref(bad)),
                 "graal_map_windows")
        self._windows_bad = int(bad.value)
        self._windows_shape = (len(o), int(px_rows), pc)
        return self._windows_shape

    def map_windows_fetch(self, observed=None, expected=None, residual=None, rank_of_sub=True):
        """graal_map_windows_fetch into the given float32 [n_win, px_rows, px_cols] arrays (None: not copied); returns rank_of_sub (or
        None)."""
        rank = np.full(int(getattr(self, "n_sub_total", 0)), -1, dtype=np.int32) if rank_of_sub else None
        ptr = []
        for a in (observed, expected, residual):
            if a is not None and not (a.dtype == np.float32 and a.flags["C_CONTIGUOUS"] and a.shape == getattr(self, "_windows_shape", None)):
                raise ValueError("map_windows_fetch takes C-contiguous float32 [n_win, px_rows, px_cols] arrays of the last map_windows_compute")
            ptr.append(None if a is None else a.ctypes.data_as(_f32p))
        self._ck(self._L.graal_map_windows_fetch(self._h, ptr[0], ptr[1], ptr[2], None if rank is None else rank.ctypes.data_as(_i32p)),
                 "graal_map_windows_fetch")
        return rank

    def edit_layout(self, cuts=(), joins=()):
        """graal_edit_layout: cut the junction after every fragment of `cuts`, then apply `joins` (pairs of ends, end = 2 * fragment +
        side, of the layout after the cuts) in one call; see include/graal_hip.h for the canonical result.  Returns the status array
        (int32[len(cuts) + len(joins)], EDIT_OK everywhere).  A refused edit raises GraalError (layout unchanged) with the status array
        as its .status attribute.  Afterwards the engine is as after upload_frags of the new layout."""
        c = _c(np.asarray(cuts, dtype=np.int64).reshape(-1), np.int32)
        j = np.asarray(joins, dtype=np.int64).reshape(-1, 2)
        a, b = _c(j[:, 0], np.int32), _c(j[:, 1], np.int32)
        st = np.zeros(len(c) + len(a), dtype=np.int32)
        rc = self._L.graal_edit_layout(self._h, len(c), c.ctypes.data_as(_i32p), len(a), a.ctypes.data_as(_i32p), b.ctypes.data_as(_i32p),
                                       st.ctypes.data_as(_i32p))
        if rc != 0:
            try:
                self._ck(rc, "graal_edit_layout")
            except GraalError as err:
                err.status, err.code = st, rc
                raise
        return st

    def genome_distance_half_units(self):
        v = ctypes.c_int64(0)
        self._ck(self._L.graal_genome_distance(self._h, ctypes.byref(v)), "graal_genome_distance")
        return int(v.value)

    # -- node-local exchange through pinned host memory (one process per GPU) ------------------
    def exchange_bytes(self, world):
        b = ctypes.c_int64(0)
        self._ck(self._L.graal_exchange_bytes(int(world), ctypes.byref(b)), "graal_exchange_bytes")
        return int(b.value)

    def step_seq(self):
        """Sequence number of the last candidate evaluation of this handle."""
        s = ctypes.c_int64(0)
        self._ck(self._L.graal_attach_exchange(self._h, None, 0, 0, 1, 0, ctypes.byref(s)), "graal_attach_exchange")
        return int(s.value)

    def attach_exchange(self, shared_map, rank, world, seq_floor):
        """`shared_map`: an ``mmap`` of the segment all ranks of the node share (>= exchange_bytes(world), zero filled).
        The engine keeps it alive; from now on :meth:`eval_candidates_x` returns sums over all ranks."""
        view = ctypes.c_char.from_buffer(shared_map)
        s = ctypes.c_int64(0)
        self._ck(self._L.graal_attach_exchange(self._h, ctypes.c_void_p(ctypes.addressof(view)), len(shared_map), int(rank),
                                               int(world), int(seq_floor), ctypes.byref(s)), "graal_attach_exchange")
        self._x_map, self._x_view = shared_map, view
        return int(s.value)

    def exchange_selftest(self, tag, phase):
        """phase 0: this rank's GPU tags its slots; (barrier); phase 1: True if this host sees every rank's tag."""
        rc = self._L.graal_exchange_selftest(self._h, int(tag), int(phase))
        if phase == 0:
            self._ck(rc, "graal_exchange_selftest")
        return rc == 0

    @staticmethod
    def rccl_available():
        """True if librccl can be loaded in this process (what graal_attach_rccl needs; no communicator is made)."""
        buf = ctypes.create_string_buffer(128)
        return load().graal_rccl_unique_id(buf) == 0

    @staticmethod
    def rccl_unique_id():
        """The 128-byte id of a new RCCL communicator (rank 0 makes it, every rank attaches with it)."""
        buf = ctypes.create_string_buffer(128)
        rc = load().graal_rccl_unique_id(buf)
        if rc != 0:
            raise GraalError("graal_rccl_unique_id failed (%d): RCCL not found?" % rc)
        return bytes(buf.raw)

    def attach_rccl(self, id128, rank, world):
        """From now on the ranks' Q vectors are summed by one ncclAllReduce on the engine's stream (include/graal_hip.h)."""
        self._ck(self._L.graal_attach_rccl(self._h, ctypes.c_char_p(bytes(id128)), int(rank), int(world)), "graal_attach_rccl")

    def detach_rccl(self):
        self._ck(self._L.graal_detach_rccl(self._h), "graal_detach_rccl")

    def detach_exchange(self):
        self._ck(self._L.graal_detach_exchange(self._h), "graal_detach_exchange")
        if self._x_view is not None:
            self._x_view = None
            try:
                self._x_map.close()
            except (BufferError, ValueError):
                pass
            self._x_map = None

    def eval_candidates_x(self, fA, fB, max_id):
        """Sharded, synchronous: float64 [K, 13] = (sum over ALL ranks of the int64 sums) / 2^30; every rank calls it."""
        K = len(fB)
        if 1 <= K <= MAX_NEIGHBOURS:
            self._fb_buf[:K] = fB
            rc = self._L.graal_eval_candidates_x(self._h, int(fA), self._fb_ptr, K, int(max_id), self._q_ptr, self._c_ptr)
            if rc != 0:
                self._ck(rc, "graal_eval_candidates_x")
            return q_to_float(self._q_buf[:K * N_OPS], self._c_buf[:K * N_OPS]).reshape(K, N_OPS)
        fb = _c(fB, np.int32)
        out = np.zeros((len(fb), N_OPS), dtype=np.float64)
        for k0 in range(0, len(fb), MAX_NEIGHBOURS):
            out[k0:k0 + MAX_NEIGHBOURS] = self.eval_candidates_x(fA, fb[k0:k0 + MAX_NEIGHBOURS], max_id)
        return out

    def eval_candidates_q_async(self, fA, fB, max_id, d_out_ptr, stream_ptr, rank=0, world=1):
        """Asynchronous Q-valued form for the multi-GPU path: K*13 int64 into a DEVICE buffer on `stream`."""
        fb = _c(fB, np.int32)
        assert 1 <= len(fb) <= MAX_NEIGHBOURS
        self._ck(self._L.graal_eval_candidates_q(self._h, int(fA), fb.ctypes.data_as(_i32p), len(fb), int(max_id),
                                                 int(rank), int(world), ctypes.c_void_p(int(d_out_ptr)),
                                                 ctypes.c_void_p(int(stream_ptr) if stream_ptr else 0)),
                 "graal_eval_candidates_q")

    # -- the per-step host logic in C (graal_step) ---------------------------------------------------
    def upload_proposal_tables(self, xk, pk, id_d, dispatcher, collector, dup_bin_flags, black_frag_flags):
        xk = _c(xk, np.int32); pk = _c(pk, np.float32)
        idd = _c(id_d, np.int32); disp = _c(np.asarray(dispatcher).reshape(-1, 2), np.int32); coll = _c(collector, np.int32)
        dup = _c(dup_bin_flags, np.uint8); blk = _c(black_frag_flags, np.uint8)
        assert xk.shape == pk.shape and len(dup) == xk.shape[0] == len(disp) and len(blk) == len(idd)
        u8 = ctypes.POINTER(ctypes.c_uint8)
        self._ck(self._L.graal_upload_proposal_tables(self._h, xk.ctypes.data_as(_i32p), pk.ctypes.data_as(_f32p), xk.shape[0], xk.shape[1],
                                                      idd.ctypes.data_as(_i32p), len(idd), disp.ctypes.data_as(_i32p),
                                                      coll.ctypes.data_as(_i32p), len(coll), dup.ctypes.data_as(u8), blk.ctypes.data_as(u8)),
                 "graal_upload_proposal_tables")
        self.step_out = StepOut()
        self._step_ref = ctypes.byref(self.step_out)
        self.step_scores = np.frombuffer(self.step_out, dtype=np.float64, count=128 * N_OPS, offset=StepOut.scores.offset)

    def step(self, mt_addr, fA, delta, likelihood_t, flags, prev_circ):
        """graal_step: STEP_DONE / STEP_PAUSED / STEP_FALLBACK / STEP_SELECT; results in self.step_out"""
        rc = self._L.graal_step(self._h, mt_addr, fA, delta, likelihood_t, flags, prev_circ, self._step_ref)
        if rc >= 16:
            self._ck(rc - 16, "graal_step")
        return rc

    def steps(self, mt_addr, ids, delta, likelihood_t, flags, prev_circ):
        """graal_steps: a run of steps in one call.  Returns (rc of the last step started, rows[n_done, STEPS_ROW]); a step that
        did not end STEP_DONE has left its state in self.step_out, like step()."""
        ids = _c(ids, np.int32)
        rows = np.empty((len(ids), STEPS_ROW), dtype=np.float64)
        n_done = ctypes.c_int32(0)
        rc = self._L.graal_steps(self._h, mt_addr, ids.ctypes.data_as(_i32p), len(ids), delta, likelihood_t, flags, prev_circ,
                                 rows.ctypes.data_as(_f64p), ctypes.byref(n_done), self._step_ref)
        if rc >= 16:
            self._ck(rc - 16, "graal_steps")
        return rc, rows[:n_done.value]

    def step_finish(self, mt_addr, likelihood_t, flags):
        rc = self._L.graal_step_finish(self._h, mt_addr, likelihood_t, flags, self._step_ref)
        if rc >= 16:
            self._ck(rc - 16, "graal_step_finish")
        return rc

    def set_finisher(self, enabled):
        """Let the table kernel's last block finish short-contig steps (default) or always use the finishing kernel."""
        self._ck(self._L.graal_set_finisher(self._h, 1 if enabled else 0), "graal_set_finisher")

    def set_mode(self, ref_trans_accu=False, strict=False):
        """Reference-arithmetic switches (include/graal_hip.h: GRAAL_MODE_REF_TRANS_ACCU = 1, GRAAL_MODE_STRICT = 2)."""
        self._ck(self._L.graal_set_mode(self._h, (MODE_REF_TRANS_ACCU if ref_trans_accu else 0) | (MODE_STRICT if strict else 0)),
                 "graal_set_mode")

    def set_timing(self, enabled):
        self._ck(self._L.graal_set_timing(self._h, int(enabled)), "graal_set_timing")

    def set_scan_path(self, path):
        """graal_set_scan_path: 0 = the engine chooses per step, 1 = always stream the contact list, 2 = always take the step's contacts
        through the row index (an error where that is not possible)."""
        self._ck(self._L.graal_set_scan_path(self._h, int(path)), "graal_set_scan_path")

    def last_timing(self):
        t = np.zeros(4, dtype=np.float32)
        self._ck(self._L.graal_last_timing(self._h, t.ctypes.data_as(_f32p)), "graal_last_timing")
        return t

    def scan_times(self, n):
        """k_scan durations (ms) of the last n candidate evaluations (HIP event pairs recorded around each launch)."""
        t = np.zeros(int(n), dtype=np.float32)
        self._ck(self._L.graal_scan_times(self._h, int(n), t.ctypes.data_as(_f32p)), "graal_scan_times")
        return t

    def strict_times(self, n):
        """Durations (ms) of the tiled reference-arithmetic kernel (k_strict2) in the last n evaluations that carried an event pair."""
        t = np.zeros(int(n), dtype=np.float32)
        self._ck(self._L.graal_strict_times(self._h, int(n), t.ctypes.data_as(_f32p)), "graal_strict_times")
        return t

    def time_scan(self, K, reps=50):
        """Average k_scan duration (ms) over `reps` back-to-back replays between two HIP events."""
        ms = ctypes.c_float(0.0)
        self._ck(self._L.graal_time_scan(self._h, int(K), int(reps), ctypes.byref(ms)), "graal_time_scan")
        return float(ms.value)

    def take_carry_correction(self):
        """graal_take_carry_correction: (correction in log-likelihood units, valid) of the commits since the last take."""
        q, v = ctypes.c_int64(0), ctypes.c_int32(0)
        self._ck(self._L.graal_take_carry_correction(self._h, ctypes.byref(q), ctypes.byref(v)), "graal_take_carry_correction")
        return float(q.value) / Q_SCALE, bool(v.value)

    def upload_own_obs(self, own):
        """graal_upload_own_obs: float32 [n_bins, 3], the observed counts of every bin's own sub-fragment pairs over the WHOLE contact list."""
        own = _c(own, np.float32)
        assert own.ndim == 2 and own.shape[1] == 3
        self._ck(self._L.graal_upload_own_obs(self._h, own.ctypes.data_as(_f32p), own.shape[0]), "graal_upload_own_obs")

    def explode(self):
        """graal_explode: explode_genome's loop (relabel + eject, fragment by fragment) as one call; returns the stale-paste count."""
        v = ctypes.c_int64(0)
        self._ck(self._L.graal_explode(self._h, ctypes.byref(v)), "graal_explode")
        return int(v.value)

    def discard_carry_correction(self):
        """The caller holds a full evaluation of the current layout: the corrections of the commits up to it are void."""
        self._ck(self._L.graal_take_carry_correction(self._h, None, None), "graal_take_carry_correction")

    def run_counters(self):
        """include/graal_hip.h: graal_run_counters -- evaluations, repeats behind events (`fallbacks`), in-kernel waits in use,
        k_strict2 launches behind k_gprep's word / behind the event, k_strict_flat launches, hand-overs to a finishing kernel, finisher give-ups,
        ..., evaluations whose contacts came through the row index (`indexed_passes`)."""
        c = np.zeros(12, dtype=np.int64)
        self._ck(self._L.graal_run_counters(self._h, c.ctypes.data_as(_i64p)), "graal_run_counters")
        return dict(zip(("evaluations", "fallbacks", "in_kernel_waits_in_use", "strict2_behind_the_word", "strict2_behind_the_event",
                         "flat_launches", "handed_to_a_finishing_kernel", "finisher_gave_up", "unit_list_grown", "unit_list_capacity",
                         "carried_totals_repaired", "indexed_passes"),
                        (int(x) for x in c[:12])))

    def last_counters(self):
        c = np.zeros(4, dtype=np.int64)
        self._ck(self._L.graal_last_counters(self._h, c.ctypes.data_as(_i64p)), "graal_last_counters")
        return c
