"""Stored outputs of the linked reference (oracle/_ref) for the tests that compare against it.

A test hands reference_outputs() a name and a function that computes, through the linked
reference, every value the test compares with: a dict of arrays.  Where oracle/_ref is built the
function runs live and its result must equal the stored copy in tests/golden/ref/<name>.npz (with
EPV_WRITE_REF_GOLDEN=1 the copy is written instead); everywhere else the stored copy stands in for
the reference, so the same assertions run on a checkout that has only the repository."""
import os

import numpy as np

import orc
from common import GOLDEN
from epievo_amd import host

REF_GOLDEN = os.path.join(GOLDEN, "ref")


def reference_outputs(name, compute):
    path = os.path.join(REF_GOLDEN, name + ".npz")
    if not orc.have_ref():
        with np.load(path) as z:
            return {k: z[k] for k in z.files}
    live = {k: np.asarray(v) for k, v in compute().items()}
    if os.environ.get("EPV_WRITE_REF_GOLDEN") == "1":
        os.makedirs(REF_GOLDEN, exist_ok=True)
        np.savez_compressed(path, **live)
        return live
    with np.load(path) as z:
        assert sorted(z.files) == sorted(live), (name, sorted(z.files), sorted(live))
        for k in z.files:
            assert z[k].dtype == live[k].dtype and np.array_equal(z[k], live[k]), \
                "%s: the linked reference no longer gives the stored %s" % (name, k)
    return live


def pack_paths(prefix, fp):
    """a FlatPaths as entries of a reference_outputs dict"""
    return {prefix + "_shape": np.array([fp.n_sites, fp.n_nodes], np.uint64), prefix + "_init": fp.init,
            prefix + "_offsets": fp.offsets, prefix + "_jumps": fp.jumps}


def unpack_paths(prefix, d):
    n, N = (int(x) for x in d[prefix + "_shape"])
    return host.FlatPaths(n, N, d[prefix + "_init"], d[prefix + "_offsets"], d[prefix + "_jumps"])


def pack_text(s):
    return np.frombuffer(s.encode() if isinstance(s, str) else s, np.uint8).copy()


def unpack_text(a):
    return bytes(np.asarray(a, np.uint8)).decode()
