#!/usr/bin/env python3
"""Generates tests/golden/ref_mutations.npz, ref_likelihood.npz and ref_likelihood_params.npz: what the REFERENCE'S OWN kernels,
compiled for the host (oracle/ref_kernels.py; needs oracle/_ref/libgraal_ref.so, i.e. the reference's sources), give for the cases
of tests/ref_cases.py -- the last under the parameter sets of tests/param_cases.py.  The GPU tests read these files, never the
library.  Run from the repo root:
python tests/golden/make_ref_fixtures.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle.ref_kernels import RefKernels  # noqa: E402
from tests import ref_cases  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
LIMIT = 128187   # the largest fixture committed before these (rippe_fit.json)


def main():
    if not RefKernels.available():
        sys.exit("oracle/_ref/libgraal_ref.so is missing: build it where the reference's kernels3.cu is")
    mut, lik = ref_cases.fixture_arrays(RefKernels)
    par = ref_cases.param_fixture_arrays(RefKernels)      # the parameter sets of tests/param_cases.py: totals and deltas, no pixels
    for name, arrays in (("ref_mutations.npz", mut), ("ref_likelihood.npz", lik), ("ref_likelihood_params.npz", par)):
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        print(name, size, "bytes")
        assert size <= LIMIT, (name, size)


if __name__ == "__main__":
    main()
