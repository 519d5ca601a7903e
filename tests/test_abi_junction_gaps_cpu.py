"""graal_junction_gaps is declared in the header, bound in graal_amd.lib and exported by the built library (tests/test_abi_cpu.py checks
the three lists against each other; this names the one symbol and its argument list)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_declared_bound_and_exported():
    from graal_amd import build as gbuild
    from graal_amd import lib
    header = open(os.path.join(ROOT, "include", "graal_hip.h")).read()
    m = re.search(r"^int graal_junction_gaps\(([^;]*)\);", header, re.M)
    assert m, "not declared"
    args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
    assert args == ["graal_ctx* h", "const float* gap_kb", "int32_t n_gaps", "int64_t drop_q", "int64_t* q_out", "uint8_t* status",
                    "int32_t* best", "int64_t* q_best", "int32_t* lo", "int32_t* hi", "int64_t* q_gap"]
    assert re.search(r"#define GRAAL_ABI_VERSION 7\b", header)
    assert "graal_junction_gaps" in lib.SYMBOLS
    L = ctypes.CDLL(gbuild.build_hip())
    assert getattr(L, "graal_junction_gaps") is not None
    assert callable(lib.Engine.junction_gaps) and callable(lib.Engine.junction_gaps_q)
    null = ctypes.c_void_p()
    L.graal_junction_gaps.restype = ctypes.c_int
    assert L.graal_junction_gaps(null, None, 1, 0, None, None, None, None, None, None, None) == 1      # GRAAL_E_ARG before anything else
