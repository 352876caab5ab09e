"""GetResourceUtilization (cluster.go:46-63) restated in numpy float32, the ways of summing it is
NOT, and the comparison rule of the utilization tests — shared by the oracle and the GPU tests.

The Go loop is, per resource, one float32 conversion of each operand, one float32 subtraction and
one float32 addition per node, in node order, then one float32 division by the float32 conversion
of the uint32 total (SetTotalResources, cluster.go:26-40, a wrapping sum).  Past 2^24 every one of
these rounds, so the order and the place of each conversion show in the bits.
"""
from __future__ import annotations

import numpy as np

U32 = 0xFFFFFFFF
F32 = np.float32


def terms(cap, free):
    """float32(cap_i) - float32(free_i) per node: convert each operand, then subtract."""
    cap, free = np.asarray(cap, np.uint64), np.asarray(free, np.uint64)
    return [F32(F32(c) - F32(f)) for c, f in zip(cap, free)]


def serial_sum(cap, free):
    """The Go sum: float32, node order."""
    s = F32(0)
    for x in terms(cap, free):
        s = F32(s + x)
    return s


def total_u32(cap):
    return int(np.asarray(cap, np.uint64).sum(dtype=np.uint64)) & U32


def divide(s, total):
    """float32 sum / float32(uint32 total): x/0 is +-Inf, 0/0 is NaN, as IEEE 754 and Go have it."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return F32(F32(s) / F32(total))


def utilization(cap, free):
    """One resource column of GetResourceUtilization."""
    return divide(serial_sum(cap, free), total_u32(cap))


def resource_utilization(cap_c, cap_m, free_c, free_m):
    return utilization(cap_c, free_c), utilization(cap_m, free_m)


def _tree(xs):
    if len(xs) == 0:
        return F32(0)
    if len(xs) == 1:
        return xs[0]
    h = len(xs) // 2
    return F32(_tree(xs[:h]) + _tree(xs[h:]))


def wrong_sums(cap, free):
    """The sum by four plausible wrong methods, as float32: the node order reversed, a pairwise
    tree, a float64 sum rounded once, and an integer sum converted once."""
    ts = terms(cap, free)
    rev = F32(0)
    for x in reversed(ts):
        rev = F32(rev + x)
    cap, free = np.asarray(cap, np.uint64), np.asarray(free, np.uint64)
    f64 = np.float64(0)
    for c, f in zip(cap, free):
        f64 = f64 + (np.float64(c) - np.float64(f))
    isum = sum(int(c) - int(f) for c, f in zip(cap, free))
    return {"reversed": rev, "tree": _tree(ts), "float64": F32(f64), "integer": F32(isum)}


def wrong_utilizations(cap, free):
    t = total_u32(cap)
    return {k: divide(v, t) for k, v in wrong_sums(cap, free).items()}


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def same(a, b):
    """Elementwise equality of float32 values under the NaN rule: two NaNs are equal whatever their
    sign and payload (Go fixes neither; x86 and gfx950 produce different default NaNs); everything
    else compares bit for bit, the infinities and the sign of zero included."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def discriminates(cap, free):
    """Per wrong method: does the serial utilization of this column differ from it?"""
    want = utilization(cap, free)
    return {k: not bool(same(want, v)) for k, v in wrong_utilizations(cap, free).items()}


def sums_reach_2_24(arrays):
    """Does some cluster's sum of max(capacity, availability) reach 2^24 in a resource?  Below it every
    partial sum of the float32 loop is an exact integer, and an integer sum is the same number."""
    for c in range(arrays.n_clusters):
        ns = arrays.nodes_of(c)
        for cap, free in ((arrays.cap_c, arrays.free_c), (arrays.cap_m, arrays.free_m)):
            if int(np.maximum(cap[ns], free[ns]).astype(np.uint64).sum()) >= 1 << 24:
                return True
    return False


def clusters_where_the_integer_sum_differs(arrays):
    """The clusters whose utilization sample of the loaded state (the one a trader reads before
    anything runs) is another float32 when summed in integers and converted once."""
    out = []
    for c in range(arrays.n_clusters):
        ns = arrays.nodes_of(c)
        if discriminates(arrays.cap_c[ns], arrays.free_c[ns])["integer"] or \
                discriminates(arrays.cap_m[ns], arrays.free_m[ns])["integer"]:
            out.append(c)
    return out


def w32_cluster(rng):
    """One cluster of the 'w32' fuzz range (kat_util.fuzz_workload): 129-256 nodes, a node memory
    in 40000 .. 2^30, random availability on about a third of the nodes.
    Returns (cap_c, cap_m, free_c, free_m) as uint64 arrays."""
    nn = int(rng.integers(129, 257))
    cap_c, cap_m = int(rng.integers(1, 64)), int(rng.integers(40000, 1 << 30))
    full = rng.random((2, nn)) < 0.7
    free_c = np.where(full[0], cap_c, rng.integers(0, cap_c + 1, nn)).astype(np.uint64)
    free_m = np.where(full[1], cap_m, rng.integers(0, cap_m + 1, nn)).astype(np.uint64)
    return np.full(nn, cap_c, np.uint64), np.full(nn, cap_m, np.uint64), free_c, free_m
