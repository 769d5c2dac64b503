"""A tree the file reader built (vxg_file_column_array) against the tree that was written (plain
module, shared by tests/test_vxfile.py and tests/test_file_cases.py).

With region = NULL the reader's buffer pointers are file offsets, so `check_tree` compares a
reconstructed node with the written Array node for node: encoding id, length, dtype, ptype,
nullability, validity kind, the decoded metadata, every buffer's length and bytes at its 64-byte
aligned file offset, and the child count.
"""
import numpy as np

import vortex_amd._lib as L
import vortex_amd.arrays as A
from tools import vxfile as X


def check_tree(node, a, data: np.ndarray, path="root"):
    if a.encoding == X.ENC_EXTENSION:
        a = a.children[0]
    assert node.encoding == a.encoding, path
    assert node.len == a.len, path
    assert node.dtype == a.dtype, path
    if a.dtype == L.DTYPE["PRIMITIVE"]:
        assert L.PTYPES[node.ptype] == a.ptype, path
    assert bool(node.nullable) == bool(a.nullable), path
    assert node.validity == a.validity, path
    m = L.VxgMeta()
    A._fill_meta(m, a)
    assert bytes(m) == bytes(node.meta), (path, a.encoding, a.meta)
    if a.buffers:
        want = np.ascontiguousarray(a.buffers[0]).view(np.uint8).reshape(-1)
        assert node.n_buffers == 1, path
        off, n = int(node.buffers[0].ptr or 0), int(node.buffers[0].len)
        assert off % 64 == 0, path  # 64-byte aligned in the file (lib.rs:15)
        assert n == want.size, path
        assert data[off: off + n].tobytes() == want.tobytes(), path
    else:
        assert node.n_buffers == 0, path
    assert node.n_children == len(a.children), path
    for i, c in enumerate(a.children):
        check_tree(node.children[i], c, data, f"{path}/{i}")


def leaf_buffers(node):
    """(pointer, length) of every buffer of the reader's tree under `node`."""
    out = [(int(node.buffers[i].ptr or 0), int(node.buffers[i].len)) for i in range(node.n_buffers)]
    for i in range(node.n_children):
        out += leaf_buffers(node.children[i])
    return out
