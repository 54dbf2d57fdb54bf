# coding: utf-8
"""Meshes that pin the one probe loop of csrc/dudf_meshtab.h through the three mesh units (tests/test_meshclean_gpu.py,
test_meshtopo_gpu.py, test_simplify_gpu.py).  Test infrastructure only.  The hash is restated in numpy, and `wrap_mesh` asserts what
it was built for as its own precondition: after a change of hash or capacity the tests fail here instead of passing idly."""
import numpy as np

import meshtopo_oracle as T

WRAP_FACES = np.array([[18, 23, 28], [6, 32, 39], [1, 15, 35], [5, 7, 34]], np.int64)
WRAP_H = 0.5                                                                   # a lattice on which every vertex has its own cell


def mix64(x):
    """splitmix64's finaliser over uint64 arrays (csrc/dudf_meshtab.h: dudf_mix64)."""
    x = np.asarray(x, np.uint64).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(30); x *= np.uint64(0xbf58476d1ce4e5b9)
        x ^= x >> np.uint64(27); x *= np.uint64(0x94d049bb133111eb)
    return x ^ (x >> np.uint64(31))


def pow2_at_least(n):
    c = 2
    while c < n:
        c <<= 1
    return c


def edge_slots(faces):
    """The home slot of every undirected edge (rows of sorted pairs, once each) in the edge table of `faces`: capacity >= 6 F."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    e = np.unique(np.sort(np.stack([f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)], 1), 1), axis=0).astype(np.uint64)
    return e.astype(np.int64), (mix64((e[:, 0] << np.uint64(32)) | e[:, 1]) & np.uint64(pow2_at_least(6 * len(f)) - 1)).astype(np.int64)


def triple_slots(g):
    """The home slot of every face's sorted triple in the face table of `g`: capacity >= 2 F."""
    t = np.sort(np.asarray(g, np.int64).reshape(-1, 3), 1).astype(np.uint64)
    return (mix64(mix64((t[:, 0] << np.uint64(32)) | t[:, 1]) ^ t[:, 2]) & np.uint64(pow2_at_least(2 * len(t)) - 1)).astype(np.int64)


def wrap_mesh():
    """(vertices, faces): 40 distinct finite vertices, each alone in its cell of the lattice of edge WRAP_H at the origin, and four
    faces.  Every edge table has 32 slots and three edges have the last one as their home: the chain goes on at slots 0 and 1.  The
    clean-up's face table has 8 slots and two triples have the last one as their home."""
    i = np.arange(40)
    rng = np.random.default_rng(40)
    cell = np.stack([i, (7 * i) % 40, (11 * i) % 40], 1)                       # distinct in every coordinate
    v = (cell + 0.2 + 0.6 * rng.random((40, 3))) * WRAP_H
    f = WRAP_FACES.copy()
    edges, slots = edge_slots(f)
    assert pow2_at_least(6 * len(f)) == 32 and sorted(map(tuple, edges[slots == 31])) == [(6, 39), (18, 28), (32, 39)], (edges, slots)
    assert pow2_at_least(2 * len(f)) == 8 and (triple_slots(f) == 7).sum() == 2, triple_slots(f)
    return v, f


def edge_use_counts(faces):
    """Uses per undirected edge of valid faces without repeated indices (np.unique on sorted pairs)."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    e = np.sort(np.stack([f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)], 1), 1)
    return np.unique(e, axis=0, return_counts=True)[1]


def holed_grid(extra_face=False):
    """(vertices, faces): the 17 x 17 lattice plane (512 faces: whole workgroups) without every 37th face, and with `extra_face` a
    third face on an interior edge."""
    v, f = T.grid_plane(16, 16)
    assert len(f) == 512
    f = f[np.arange(512) % 37 != 36]
    if extra_face:
        u, w = 17 * 8 + 8, 17 * 9 + 8                                          # the edge between two lattice neighbours in mid-plane
        assert ((f == u).any(1) & (f == w).any(1)).sum() == 2
        f = np.concatenate([f, [[u, w, 0]]])                                   # vertex 0 is no neighbour of either
    return v, f
