"""TEST INFRASTRUCTURE -- the reference's own kernels, run on the CPU.  Not product code.

:class:`RefKernels` has the constructor and the methods of :class:`oracle.oracle.DenseOracle`, but every
call launches the kernel of the reference's ``kernels3.cu`` itself, compiled for the host by the recipe
``oracle/Makefile: _ref/libgraal_ref.so`` (stand-in header ``oracle/ref_host/curand_kernel.h``, launcher
``oracle/ref_host/ref_launch.cpp``).  Nothing of the reference is restated here except the order of each
kernel's arguments, which the host code of the reference fixes in the same way (``cuda_lib_gl.py``, one
PyCUDA call per kernel); the launcher reports each kernel's argument count and sizes and every launch is
checked against them.

The library exists only where the reference's sources are (``build()`` makes it there); everything that
needs it asks :func:`available` first.  GPU tests never load it: they read outputs recorded from it
(``tests/golden/ref_*.npz``).

Only the reference's trans-branch RF-count indexing exists in its text, so this class corresponds to
``DenseOracle(fix_trans_accu=False)`` and refuses ``True``.
"""
import ctypes
import os

import numpy as np

from oracle.oracle import FIELDS, _ptrs

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_ref", "libgraal_ref.so")

BLOCK = 32  # threads per block of every launch
MIN_GRID = 2  # at least two blocks, so that block-shared logic runs in more than one block
SENTINEL = -7  # prefill of paste's output; no field of a valid layout is -7

_lib = None


def available():
    """True where oracle/_ref/libgraal_ref.so has been built (the reference's sources were present)."""
    return os.path.exists(LIB_PATH)


def lib():
    global _lib
    if _lib is None:
        if not available():
            raise RuntimeError("oracle/_ref/libgraal_ref.so is not built: the reference's kernels3.cu is needed "
                               "(make -C oracle _ref/libgraal_ref.so REF=<dir>)")
        _lib = ctypes.CDLL(LIB_PATH)
    return _lib


def build(ref_dir=None):
    """What __graft_entry__.build() runs: make the library where the reference's kernels3.cu is (``ref_dir``, else the
    Makefile's REF), keep an earlier one where it is not, go on without one otherwise.  Only a MISSING reference is
    passed over: where kernels3.cu exists and the stand-in header, the launcher or the file no longer compile, the
    compiler's messages are shown and CalledProcessError is raised, so that neither a stale library stays in use nor the
    live tests skip unnoticed.  Returns available()."""
    import subprocess
    cmd = ["make", "-C", _HERE, "ref-if-present"] + (["REF=" + ref_dir] if ref_dir else [])
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL)
    return available()


_sizes = {}


def _arg_sizes(name, function=False):
    if name not in _sizes:
        buf = (ctypes.c_int * 64)()
        if function:
            rs = ctypes.c_int(0)
            n = getattr(lib(), "ref_nargs_" + name)(buf, ctypes.byref(rs))
            _sizes[name] = (list(buf[:n]), rs.value)
        else:
            n = getattr(lib(), "ref_nargs_" + name)(buf)
            _sizes[name] = (list(buf[:n]), 0)
    return _sizes[name]


def _pack(name, args, function=False):
    """void*[] of pointers to the argument values, checked against the kernel's own declaration."""
    sizes, ret = _arg_sizes(name, function)
    assert len(args) == len(sizes), (name, len(args), len(sizes))
    for i, (a, s) in enumerate(zip(args, sizes)):
        assert ctypes.sizeof(a) == s, (name, i, ctypes.sizeof(a), s)
    arr = (ctypes.c_void_p * len(args))(*[ctypes.addressof(a) for a in args])
    return arr, ret


def _launch(name, n_threads, args, shared=0, grid=None):
    if grid is None:
        grid = max(MIN_GRID, int(n_threads) // BLOCK + 1)  # n // size_block + 1, as every launch of the reference
    arr, _ = _pack(name, args)
    getattr(lib(), "ref_launch_" + name)(ctypes.c_int(grid), ctypes.c_int(BLOCK), ctypes.c_size_t(shared), arr)


def _call(name, restype, args):
    arr, ret = _pack(name, args, function=True)
    out = restype()
    assert ctypes.sizeof(out) == ret, (name, ret)
    getattr(lib(), "ref_call_" + name)(ctypes.byref(out), arr)
    return out.value


def _i(v):
    return ctypes.c_int(int(v))


def _p(a):
    """A device pointer argument: the address of a numpy array (kept alive by the caller)."""
    return ctypes.c_void_p(a.ctypes.data)


class _Frag:
    """struct frag: 14 pointers in FIELDS order; the kernels take its address.

    paste_contigs and pop_in_frag_1..4 read the source entry [threadIdx.x + blockDim.x * blockIdx.x] of every field BEFORE
    they test it against n_frags (kernels3.cu:1841-1853, 644 ff.), so the threads past the last fragment read beyond the
    arrays (found by the stand-alone self-test under the address sanitizer; harmless on a GPU, where the values are never
    used).  Every layout therefore travels as a zero-padded copy of one entry per launched thread, and ``back`` returns
    the first n entries of an output."""

    def __init__(self, state):
        n = len(state["pos"])
        size = max(MIN_GRID, n // BLOCK + 1) * BLOCK
        self.copy = {k: np.zeros(size, dtype=np.int32) for k in FIELDS}
        for k in FIELDS:
            self.copy[k][:n] = state[k]
        self.ptrs = _ptrs(self.copy)
        self.arg = ctypes.c_void_p(ctypes.addressof(self.ptrs))

    def back(self, state):
        n = len(state["pos"])
        for k in FIELDS:
            state[k][:] = self.copy[k][:n]


class _Param(ctypes.Structure):
    _pack_ = 1
    _fields_ = [(k, ctypes.c_float) for k in ("kuhn", "lm", "c1", "slope", "d", "d_max", "fact", "v_inter")]


def _param(p):
    return _Param(*[float(x) for x in np.asarray(p, dtype=np.float32).reshape(8)])


class RefKernels:
    """Dense data + the reference's kernels themselves, one call per kernel launch."""

    def __init__(self, obs, sub_id, sub_len, sub_accu, dispatcher, collector, n_bins, nfpb, param,
                 fix_trans_accu=False):
        if fix_trans_accu:
            raise ValueError("the reference's text has only its own trans-branch RF-count indexing: "
                             "RefKernels is fix_trans_accu=False")
        self.fix_trans_accu = 0
        self.obs = np.ascontiguousarray(obs, dtype=np.float32)
        assert self.obs.ndim == 2 and self.obs.shape[0] == self.obs.shape[1]
        self.width = int(self.obs.shape[0])
        # int4 / float3 / int3 / int2 device arrays, laid out as the reference uploads them
        self.sub_id = np.ascontiguousarray(sub_id, dtype=np.int32).reshape(-1, 4)
        self.sub_len = np.ascontiguousarray(sub_len, dtype=np.float32).reshape(-1, 3)
        self.sub_accu = np.ascontiguousarray(sub_accu, dtype=np.int32).reshape(-1, 3)
        self.dispatcher = np.ascontiguousarray(dispatcher, dtype=np.int32).reshape(-1, 2)
        self.collector = np.ascontiguousarray(collector, dtype=np.int32)
        self.n_bins = int(n_bins)
        self.nfpb = np.float32(nfpb)
        self.set_param(param)
        self.n_up = self.n_bins * (self.n_bins - 1) // 2
        self.n_pix = self.n_up + self.n_bins

    def set_param(self, param):
        self.param = np.ascontiguousarray(np.asarray(param, dtype=np.float32).reshape(8))

    # -- mutation kernels -------------------------------------------------------------------
    @staticmethod
    def copy(dst, src, id_contigs=None):
        n = len(src["pos"])
        d, s = _Frag(dst), _Frag(src)
        if id_contigs is None:
            _launch("simple_copy", n, [d.arg, s.arg, _i(n)])
        else:
            _launch("copy_struct", n, [d.arg, s.arg, _p(id_contigs), _i(n)])
        d.back(dst)

    @staticmethod
    def flip(dst, src, f):
        n = len(src["pos"])
        d, s = _Frag(dst), _Frag(src)
        _launch("flip_frag", n, [d.arg, s.arg, _i(f), _i(n)])
        d.back(dst)

    @staticmethod
    def swap_activity(dst, src, f, max_id):
        n = len(src["pos"])
        d, s = _Frag(dst), _Frag(src)
        _launch("swap_activity_frag", n, [d.arg, s.arg, _i(f), _i(max_id), _i(n)])
        d.back(dst)

    @staticmethod
    def pop_out(dst, src, id_contigs, f, max_id):
        n = len(src["pos"])
        d, s = _Frag(dst), _Frag(src)
        _launch("pop_out_frag", n, [d.arg, s.arg, _p(id_contigs), _i(f), _i(max_id), _i(n)])
        d.back(dst)

    @staticmethod
    def pop_in(which, dst, src, f_pop, f_ins, max_id, ori):
        assert which in (1, 2, 3, 4)
        n = len(src["pos"])
        d, s = _Frag(dst), _Frag(src)
        _launch("pop_in_frag_%d" % which, n, [d.arg, s.arg, _i(f_pop), _i(f_ins), _i(max_id), _i(ori), _i(n)])
        d.back(dst)

    @staticmethod
    def split(dst, src, id_contigs, f_cut, upstream, max_id):
        n = len(src["pos"])
        d, s = _Frag(dst), _Frag(src)
        _launch("split_contig", n, [d.arg, s.arg, _p(id_contigs), _i(f_cut), _i(upstream), _i(max_id), _i(n)])
        d.back(dst)

    @staticmethod
    def paste(dst, src, fA, fB, max_id, written=None):
        """paste_contigs.  Returns the number of entries the kernel did not write (the stale slot of its
        same-contig branch); ``written`` (bool[n]), if given, receives the mask of the entries it wrote.
        The kernel runs on a scratch output prefilled with a sentinel; only written entries reach ``dst``."""
        n = len(src["pos"])
        tmp = {k: np.full(n, SENTINEL, dtype=np.int32) for k in FIELDS}
        d, s = _Frag(tmp), _Frag(src)
        _launch("paste_contigs", n, [d.arg, s.arg, _i(fA), _i(fB), _i(max_id), _i(n)])
        d.back(tmp)
        touched = np.zeros(n, dtype=bool)
        for k in FIELDS:
            touched |= tmp[k] != SENTINEL
        whole = np.ones(n, dtype=bool)
        for k in FIELDS:
            whole &= tmp[k] != SENTINEL
        assert np.array_equal(touched, whole), "an entry is written in all of its 14 fields or in none"
        for k in FIELDS:
            dst[k][touched] = tmp[k][touched]
        if written is not None:
            written[:] = touched
        return int(n - touched.sum())

    @staticmethod
    def fill_sub_index(src, sub_index, contig, offset):
        n = len(src["pos"])
        s = _Frag(src)
        if int(offset) == 0:  # the reference fills contig A's part with _fA and contig B's, behind it, with _fB
            _launch("fill_sub_index_fA", n, [s.arg, _p(sub_index), _i(contig), _i(n)])
        else:
            _launch("fill_sub_index_fB", n, [s.arg, _p(sub_index), _i(contig), _i(offset), _i(n)])

    @staticmethod
    def relabel(state, old_2_new, id_contigs=None):
        """The contig relabel is half of the reference's display kernel gl_update_pos, which is not under
        test; this is the oracle's statement of that half (kernels3.cu:3848-3851)."""
        o2n = np.asarray(old_2_new, dtype=np.int32)
        state["id_c"][:] = o2n[state["id_c"]]
        if id_contigs is not None:
            id_contigs[:] = state["id_c"]

    # -- likelihood kernels -----------------------------------------------------------------
    def _tables(self):
        return [_p(self.collector), _p(self.dispatcher), _p(self.sub_id)]

    def evaluate(self, state, per_pixel=None):
        """evaluate_likelihood + the host's sum over the per-pixel vector (cuda_lib_gl.py:1828-1848).
        Returns the total; fills per_pixel (float64[n_pix])."""
        pp = per_pixel if per_pixel is not None else np.zeros(self.n_pix, dtype=np.float64)
        assert pp.dtype == np.float64 and pp.shape == (self.n_pix,) and pp.flags["C_CONTIGUOUS"]
        fr = _Frag(state)
        par = _param(self.param)
        args = [_p(self.obs), fr.arg, _p(self.collector), _p(self.dispatcher), _p(self.sub_id),
                _p(self.sub_id),  # rep_id_sub_frags: declared, never read
                _p(self.sub_len), _p(self.sub_accu), _p(pp), ctypes.c_void_p(ctypes.addressof(par)),
                _i(self.n_up), _i(self.n_pix), _i(self.n_bins), _i(self.width), ctypes.c_float(self.nfpb)]
        # grid-stride kernel: the reference launches fewer threads than pixels too (grid = n_block / stride)
        _launch("evaluate_likelihood", self.n_pix, args, grid=MIN_GRID)
        return float(np.sum(pp, dtype=np.float64))

    def sub_compute(self, state, sub_index_no_rep, list_rep, list_uniq, curr_likelihood):
        """sub_compute_likelihood with the host sequence of cuda_lib_gl.py:2457-2538: the four pixel ranges,
        the [-1] placeholders for empty lists, size_shared = 8 bytes per thread, the result in a zeroed
        double the kernel adds to."""
        no_rep = np.ascontiguousarray(sub_index_no_rep, dtype=np.int32)
        rep = np.ascontiguousarray(list_rep, dtype=np.int32)
        uniq = np.ascontiguousarray(list_uniq, dtype=np.int32)
        n_rep, n_no_rep, n_uniq = len(rep), len(no_rep), len(uniq)
        if n_rep == 0:
            rep = np.array([-1], dtype=np.int32)
        if n_no_rep == 0:
            no_rep = np.array([-1], dtype=np.int32)
        if n_uniq == 0:
            uniq = np.array([-1], dtype=np.int32)
        n_intra = n_rep * (n_rep - 1) // 2
        n_vals_no_rep = n_no_rep * (n_no_rep - 1) // 2
        lim_rep_vs_uniq = n_vals_no_rep + n_rep * n_uniq
        lim_intra = lim_rep_vs_uniq + n_intra
        n_values = lim_intra + n_rep
        out = np.zeros(1, dtype=np.float64)
        fr = _Frag(state)
        par = _param(self.param)
        assert curr_likelihood.dtype == np.float64 and curr_likelihood.flags["C_CONTIGUOUS"]
        args = [_p(self.obs), fr.arg, _p(no_rep), _p(rep), _p(uniq), _p(self.collector), _p(self.dispatcher),
                _p(self.sub_id), _p(self.sub_len), _p(self.sub_accu), _p(out), _p(curr_likelihood),
                ctypes.c_void_p(ctypes.addressof(par)), _i(n_vals_no_rep), _i(lim_rep_vs_uniq), _i(lim_intra),
                _i(n_values), _i(n_uniq), _i(n_rep), _i(self.width), _i(self.n_bins), ctypes.c_float(self.nfpb)]
        _launch("sub_compute_likelihood", n_values, args, shared=BLOCK * 8, grid=MIN_GRID)
        return float(out[0])


# -- scalar device functions --------------------------------------------------------------------
def rippe(s, param):
    return float(_call("rippe_contacts", ctypes.c_float, [ctypes.c_float(s), _param(param)]))


def rippe_circ(s, s_tot, param):
    return float(_call("rippe_contacts_circ", ctypes.c_float,
                       [ctypes.c_float(s), ctypes.c_float(s_tot), _param(param)]))


def lik(ex, ob):
    return float(_call("evaluate_likelihood_double", ctypes.c_double, [ctypes.c_double(ex), ctypes.c_double(ob)]))


def factorial(n):
    return float(_call("factorial", ctypes.c_float, [ctypes.c_float(n)]))


RefKernels.available = staticmethod(available)
RefKernels.rippe = staticmethod(rippe)
RefKernels.rippe_circ = staticmethod(rippe_circ)
RefKernels.lik = staticmethod(lik)
RefKernels.factorial = staticmethod(factorial)
