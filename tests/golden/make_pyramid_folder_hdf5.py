#!/usr/bin/env python3
"""Write tests/golden/pyramid_folder.hdf5 with REAL h5py: the pyramid.hdf5 that the reference keeps in a pyramid folder
(pyramid_sparse.py:83-126, 313-322), for the toy dataset of tests/test_pyramid.py::test_pyramid_folder_with_the_references_hdf5_file
(make_dataset with RandomState(5), build_and_filter(base, 3, 3)).  Its levels are those of the pyramid.npz that graal_amd/pyramid.py
builds from the same dataset, written with the reference's calls: create_group(str(level)), create_dataset('data', (3, n), 'i'),
create_dataset('nfrags', (1, 1), 'i'), attrs[str(level)] = 'done'.

h5py is not needed by the repository's own interpreter; run this, from the repository root, under one that has it:

    python tests/golden/make_pyramid_folder_hdf5.py
"""
import os
import sys
import tempfile

import h5py
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from graal_amd import pyramid as pyr              # noqa: E402
from tests.test_pyramid import make_dataset      # noqa: E402

path = os.path.join(HERE, "pyramid_folder.hdf5")
with tempfile.TemporaryDirectory() as tmp:
    base = os.path.join(tmp, "ds")
    make_dataset(base, np.random.RandomState(5))
    P = pyr.build_and_filter(base, 3, 3)
    d = dict(np.load(os.path.join(P.pyramid_folder, "pyramid.npz")))
if os.path.exists(path):
    os.remove(path)
f = h5py.File(path, "w")
for level in range(3):
    g = f.create_group(str(level))
    a = d["%d/data" % level]
    ds = g.create_dataset("data", a.shape, "i")
    ds[0, :] = a[0]
    ds[1, :] = a[1]
    ds[2, :] = a[2]
    nf = g.create_dataset("nfrags", (1, 1), "i")
    nf[:] = int(d["%d/nfrags" % level])
    f.attrs[str(level)] = "done"
f.close()
print("wrote", path, os.path.getsize(path), "bytes")
