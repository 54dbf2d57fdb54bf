# coding: utf-8
"""numpy model of the ordered sum (csrc/dudf_ordsum.h): the order in which the device adds the n rows of a double
sum, addition by addition, so that a device result can be compared bit for bit.

  groups = clamp(ceil(n / 256), 1, 256) workgroups of 256 threads;
  thread t of group b adds rows b*256 + t + k*groups*256 in ascending k, starting from +0.0;
  the workgroup adds its threads in a halving tree, strides 128 .. 1: s[t] += s[t + stride] for t < stride;
  the partials of the groups are added in index order, starting from +0.0.

A row the kernel skips (a NaN distance, a non-finite mean) is a row of +0.0 here: x + 0.0 == x for every x the kernels add.
Beside it, the orders a device sum might take by mistake, for the tests that show the inputs tell them apart."""
import numpy as np

from diffudf_amd import synth

BLOCK = 256
MAX_GROUPS = 256


def groups(n):
    return min(max(-(-int(n) // BLOCK), 1), MAX_GROUPS)


def thread_sums(x):
    """(groups, 256) float64: what every thread holds after its rows."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    g = groups(len(x))
    stride = g * BLOCK
    trips = max(-(-len(x) // stride), 1)
    rows = np.zeros(trips * stride, dtype=np.float64)
    rows[:len(x)] = x
    rows = rows.reshape(trips, g, BLOCK)
    acc = np.zeros((g, BLOCK), dtype=np.float64)
    for k in range(trips):
        acc = acc + rows[k]
    return acc


def halving_tree(acc, width=BLOCK):
    """Element 0 of every row after s[t] += s[t + stride], stride = width/2 .. 1, over the first `width` columns."""
    s = np.array(acc[:, :width], dtype=np.float64)
    stride = width // 2
    while stride > 0:
        s[:, :stride] = s[:, :stride] + s[:, stride:2 * stride]
        stride //= 2
    return s[:, 0]


def in_order(values):
    total = 0.0
    for v in np.asarray(values, dtype=np.float64).tolist():
        total += v
    return total


def partials(x):
    return halving_tree(thread_sums(x))


def ordered_sum(x):
    """The device's sum of x, a Python float."""
    with np.errstate(invalid="ignore", over="ignore"):
        return in_order(partials(x))


# ---- other orders (never the device's) --------------------------------------------------------------------------------------------
def pairwise_sum(x):
    return float(np.sum(np.asarray(x, dtype=np.float64)))


def left_to_right_sum(x):
    return in_order(x)


def butterfly_sum(x):
    """The same rows per thread, but every wave of 64 reduced by an xor butterfly (offsets 32 .. 1) and the four wave totals added
    in order: what a shuffle-based workgroup reduction would give."""
    acc = thread_sums(x)
    waves = np.stack([halving_tree(acc[:, w * 64:(w + 1) * 64], 64) for w in range(BLOCK // 64)], axis=1)
    return in_order([in_order(row) for row in waves])


def bits(value):
    return int(np.array([value], dtype=np.float64).view(np.uint64)[0])


# ---- the inputs of the pinned quantities ------------------------------------------------------------------------------------------
SIZES = (1, 255, 256, 257, 1000, 65793)          # 65 793 = 256 * 256 + 257: the first size at which some threads take a second trip
OUTLIER_K = 4
# The seed of every input at every size, found by search: sums of non-negative numbers differ between two orders by an ulp or two at
# most, and often not at all, so most seeds leave some order undecided.  These are the first at which every pinned quantity has other
# bits under the ordered sum than under numpy's pairwise sum, a left-to-right sum and a four-wave butterfly
# (tests/test_ordered_sum_cpu.py checks exactly that; one row has only one order).
DISTANCE_SEEDS = {1: 1, 255: 98, 256: 93, 257: 36, 1000: 86, 65793: 29}
TRIANGLE_SEEDS = {1: 1, 255: 2, 256: 5, 257: 5, 1000: 64, 65793: 3}
KNN_SEEDS = {1: 1, 255: 24, 256: 81, 257: 35, 1000: 56, 65793: 1}


def distance_vector(n, seed=None):
    """(n,) float32 over sixty binary orders of magnitude, 2^(-60 u) (0.5 + 0.5 v): distances of ordinary range add exactly in
    double, in every order, and would pin nothing."""
    seed = DISTANCE_SEEDS[n] if seed is None else seed
    u, v = synth.uniform01(seed, 1, 0, n), synth.uniform01(seed, 2, 0, n)
    return (2.0 ** (-60.0 * u) * (0.5 + 0.5 * v)).astype(np.float32)


def triangles(n, seed=None):
    """(vertices (3n,3) float64, faces (n,3) int64): n separate triangles in the unit cube."""
    seed = TRIANGLE_SEEDS[n] if seed is None else seed
    return synth.uniform01(seed, 3, 0, 9 * n).reshape(3 * n, 3), np.arange(3 * n, dtype=np.int64).reshape(n, 3)


def knn_distances(n, seed=None):
    """(n, OUTLIER_K) float32 squared distances; from 255 rows on, row 3 has no finite slot (+inf: it stays out of the statistics)
    and row 7 one padded slot."""
    seed = KNN_SEEDS[n] if seed is None else seed
    d = (1e-4 * synth.uniform01(seed, 4, 0, n * OUTLIER_K) ** 2).astype(np.float32).reshape(n, OUTLIER_K)
    if n >= 255:
        d[3, :] = np.inf
        d[7, OUTLIER_K - 1] = np.inf
    return d


def outlier_statistics(mean_dist, std_ratio, total=ordered_sum):
    """(mu, sigma, threshold) of the finite entries of mean_dist (n,) float64 as dudf_cloud_outliers forms them: two ordered sums
    (`total`: the sum to use), the products (m - mu)^2 and std_ratio * sigma rounded before they are added."""
    m = np.asarray(mean_dist, dtype=np.float64)
    fin = np.isfinite(m)
    count = float(fin.sum())
    with np.errstate(all="ignore"):
        mu = np.float64(total(np.where(fin, m, 0.0))) / np.float64(count)
        d = np.where(fin, m, mu) - mu
        sigma = np.sqrt(np.float64(total(d * d)) / np.float64(count))
        return float(mu), float(sigma), float(mu + np.float64(std_ratio) * sigma)
