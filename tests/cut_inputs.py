"""Seeded cost planes of the two-label cut tests (tests/test_gpu_parity.py, tests/test_cut_batch.py) and the batches test_cut_batch.py cuts in one call.

A window is (kind, seed): its planes depend on nothing else, so the same window can stand anywhere in any batch.  Kinds: the three generators of
cut_case; `swapped:<kind>`, the same planes with d0 and d1 exchanged (the opposite orientation of the push-relabel, the negated labelling); `equal`
(d0 == d1: neither terminal has a node); `one_pixel` (one node of the scarcer terminal)."""
import numpy as np

import slowflow_amd as sfa


def cut_case(rng, w, h, kind):
    st = sfa.stride_of(w)
    d0, d1 = np.zeros((h, st), np.float32), np.zeros((h, st), np.float32)
    if kind == "noise":
        d0[:, :w] = rng.uniform(0, 2, (h, w)); d1[:, :w] = rng.uniform(0, 2, (h, w))
    elif kind == "blobs":       # the typical shape: label 0 preferred everywhere except in a few compact regions
        d0[:, :w] = rng.uniform(0, 0.2, (h, w)); d1[:, :w] = 1.0 + rng.uniform(0, 0.2, (h, w))
        for _ in range(6):
            cx, cy, r = rng.integers(0, w), rng.integers(0, h), rng.integers(2, 9)
            yy, xx = np.mgrid[0:h, 0:w]
            d0[:, :w][(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] += rng.uniform(1.0, 4.0)
    else:                       # "stripes": long thin structures, long residual paths
        d0[:, :w] = 0.1; d1[:, :w] = 0.6
        d0[::7, :w] += 3.0; d1[3::7, :w] += 3.0
        d0[:, :w] += rng.uniform(0, 0.05, (h, w))
    return d0, d1


SWAP = "swapped:"


def swapped(kind):
    return SWAP + kind


def window(w, h, kind, seed):
    """(d0, d1) of one window, [h, stride] each; the stride padding is 0"""
    if kind.startswith(SWAP):
        d0, d1 = window(w, h, kind[len(SWAP):], seed)
        return d1, d0
    if kind in ("equal", "one_pixel"):
        st = sfa.stride_of(w)
        d0, d1 = np.zeros((h, st), np.float32), np.zeros((h, st), np.float32)
        if kind == "equal":
            d0[:, :w] = 0.5; d1[:, :w] = 0.5
        else:
            d0[:, :w] = 0.1; d1[:, :w] = 0.6
            d0[h // 2, w // 2] = 50.0
        return d0, d1
    return cut_case(np.random.default_rng(seed), w, h, kind)


def flip_of(d0, d1, w):
    """the orientation k_cut_count / k_cut_init choose, from the inputs alone: fewer pixels prefer label 1 -> push from them"""
    u = d1[:, :w] - d0[:, :w]
    return int((u < 0).sum() < (u > 0).sum())


# ---- shapes: the smallest that reach each piece of the 64 x 16 tiling (coloured 2 x 2, launched over ceil(tiles / 2) blocks per axis) ----------------------
SHAPES = [(130, 35),    # 3 x 3 tiles: a centre tile with four neighbours, slivers 2 px wide and 3 px tall
          (193, 49),    # 4 x 4 tiles: every block of the colour grid has all four colours
          (65, 17),     # 2 x 2 tiles, one pixel beyond the first
          (64, 16),     # one tile
          (5, 4)]
BASE = ["noise", "blobs", "stripes"]


def mixed_batch(w, h, nb, rot=0):
    """nb in {2, 3, 7}: neighbouring windows differ, a kind stands next to its swapped twin; `equal` and `one_pixel` wherever there is room for them
    (two windows hold the twins only, three hold one_pixel as the twins)"""
    s = w * h
    b0, b1, b2 = (BASE[(rot + i) % 3] for i in range(3))
    if nb == 2:
        return [(b0, s), (swapped(b0), s)]
    if nb == 3:
        return [("equal", s), ("one_pixel", s), (swapped("one_pixel"), s)]
    assert nb == 7
    return [(b0, s), (swapped(b0), s), ("equal", s), (b1, s), ("one_pixel", s), (b2, s), (swapped(b2), s)]


MIXED = [(w, h, nb, alpha) for (w, h) in SHAPES for nb in (2, 3, 7) for alpha in (0.5, 0.1)] + [(130, 35, nb, 0.0) for nb in (2, 3, 7)]


def mixed_of(w, h, nb, alpha):
    return mixed_batch(w, h, nb, rot=SHAPES.index((w, h)) + int(alpha * 10))


CYCLE = ["blobs", "noise", "equal", "stripes", "one_pixel", swapped("blobs"), swapped("noise"), swapped("one_pixel"), swapped("stripes")]
CYCLE_STEP = 4                  # coprime to len(CYCLE): every kind comes up, neighbours differ, and a kind meets its twin four windows on


def many_batch(w, h, nb):
    """kinds cycled with a stride coprime to their number; the k-th pass through the cycle draws from seed w * h + k, twins from the same"""
    n = len(CYCLE)
    return [(CYCLE[(CYCLE_STEP * b) % n], w * h + b // n) for b in range(nb)]


# 64 windows x 9 tiles: the tail-batch bound few_tiles = max(8, tiles * nb / 64) leaves its floor; 128 windows: every word of the per-window counts
MANY = [(130, 35, 64, 0.5), (65, 17, 128, 0.1), (65, 17, 100, 0.5)]

SCHEDULES = (130, 35, 0.5, [("blobs", 4550), (swapped("blobs"), 4550), ("noise", 4550), ("one_pixel", 4550), ("stripes", 4550)])


def all_windows():
    """every (w, h, alpha, kind, seed) the batched tests cut, once"""
    out = set()
    for (w, h, nb, alpha) in MIXED:
        out |= {(w, h, alpha, k, s) for (k, s) in mixed_of(w, h, nb, alpha)}
    for (w, h, nb, alpha) in MANY:
        out |= {(w, h, alpha, k, s) for (k, s) in many_batch(w, h, nb)}
    w, h, alpha, wins = SCHEDULES
    out |= {(w, h, alpha, k, s) for (k, s) in wins}
    return sorted(out)
