"""The streamed W16R loop's fit test as arithmetic on bytes (mcs_fa_macros.h, MCS_FA_FITBITS16C; DESIGN.md §4,
"Fit and commit"): a numpy restatement of the instructions, run on the CPU.  A node word holds free cores + 0x8000
in its low half and free memory + 0x8000 in its high half, a request word the clamped cores and memory, and
v_pk_sub_u16 leaves bit 15 of a half set exactly when that resource suffices (the guard bit); the 15 bits below it
are the remainder, junk to the test.  Byte c of the mask v86 must be 0xff when both guard bits of chunk c are set
and 0x00 otherwise.  Two pipelines give it:

  * four SDWA ANDs (high half & low half of each difference, gathered two chunks to a register), then one v_perm
    that sign-replicates byte 1 and byte 3 of both registers (selector 0x0b0a0908): ten vector instructions;
  * two v_perm that sign-replicate first (selector 0x0b090a08: the cores guards of two chunks into the low half,
    their memory guards into the high half), then two SDWA ANDs of high half & low half: nine.

The second is the loop's; the first is what it replaced and what the other 16-bit forms still run.  The cases pin
the selector constants and the pairing of each chunk's cores guard with its own memory guard."""
import itertools

import numpy as np

SEL_GATHER = 0x0B0A0908  # after the ANDs: byte 1, byte 3 of S1, byte 1, byte 3 of S0
SEL_CLEAN = 0x0B090A08   # before the ANDs: byte 1 of S1, of S0, byte 3 of S1, of S0
GUARD, CLAMP = 0x8000, 0x7FFF


def v_perm_b32(s0, s1, sel):
    """D.byte[i] = the byte of {S0, S1} (S1 the low dword) that selector byte i names: 0-7 the byte itself, 8-11
    the sign of byte 1, 3, 5, 7 replicated, 12 0x00, above 0xff."""
    s0, s1 = np.asarray(s0, np.uint64), np.asarray(s1, np.uint64)
    both = (s0 << np.uint64(32)) | s1
    out = np.zeros(both.shape, np.uint64)
    for i in range(4):
        k = (sel >> (8 * i)) & 0xFF
        if k <= 7:
            b = (both >> np.uint64(8 * k)) & np.uint64(0xFF)
        elif k <= 11:
            b = ((both >> np.uint64(8 * (2 * (k - 8) + 1) + 7)) & np.uint64(1)) * np.uint64(0xFF)
        else:
            b = np.full(both.shape, 0x00 if k == 12 else 0xFF, np.uint64)
        out |= b << np.uint64(8 * i)
    return out.astype(np.uint32)


def sdwa_and_halves(v):
    """v_and_b32_sdwa src0_sel:WORD_1 src1_sel:WORD_0: the 16-bit result."""
    v = np.asarray(v, np.uint32)
    return (v >> np.uint32(16)) & v & np.uint32(0xFFFF)


def words(lo, hi):
    """dst_sel:WORD_0 UNUSED_PAD, then dst_sel:WORD_1 UNUSED_PRESERVE into the same register."""
    return (lo | (hi << np.uint32(16))).astype(np.uint32)


def mask_and_then_perm(d):
    v80 = words(sdwa_and_halves(d[0]), sdwa_and_halves(d[1]))
    v81 = words(sdwa_and_halves(d[2]), sdwa_and_halves(d[3]))
    return v_perm_b32(v81, v80, SEL_GATHER)


def mask_perm_then_and(d, sel=SEL_CLEAN):
    x = v_perm_b32(d[1], d[0], sel)
    y = v_perm_b32(d[3], d[2], sel)
    return words(sdwa_and_halves(x), sdwa_and_halves(y))


def pk_sub_u16(a, b):
    a, b = np.asarray(a, np.uint32), np.asarray(b, np.uint32)
    lo = (a - b) & np.uint32(0xFFFF)
    hi = ((a >> np.uint32(16)) - (b >> np.uint32(16))) & np.uint32(0xFFFF)
    return lo | (hi << np.uint32(16))


def expected(cbits, mbits):
    out = np.zeros(np.shape(cbits[0]), np.uint32)
    for c in range(4):
        out |= (np.asarray(cbits[c] & mbits[c], np.uint32) * np.uint32(0xFF)) << np.uint32(8 * c)
    return out


def guard_combinations(junk):
    """All 256 combinations of a lane's eight guard bits, each with `junk` draws of the 15 low bits of every half.
    -> differences d[0..3], cores guards, memory guards"""
    rng = np.random.default_rng(20)
    bits = np.array(list(itertools.product((0, 1), repeat=8)), np.uint32).repeat(junk, axis=0)  # [256 * junk, 8]
    low = rng.integers(0, 1 << 15, size=bits.shape, dtype=np.uint32)
    low[::junk] = 0          # (no remainder at all)
    low[1::junk] = CLAMP     # (every low bit set)
    half = (bits << np.uint32(15)) | low
    d = [half[:, c] | (half[:, 4 + c] << np.uint32(16)) for c in range(4)]
    return d, [bits[:, c] for c in range(4)], [bits[:, 4 + c] for c in range(4)]


def test_both_pipelines_give_the_mask_for_every_guard_combination():
    d, cb, mb = guard_combinations(junk=64)
    want = expected(cb, mb)
    np.testing.assert_array_equal(mask_and_then_perm(d), want)
    np.testing.assert_array_equal(mask_perm_then_and(d), want)
    assert len(np.unique(want)) == 16  # every subset of the four chunks


def test_from_node_and_request_words():
    """The subtraction with guard bits in front: free amounts and requests at 0, 1, equal, one apart, and at the
    clamp 0x7fff, every pair of them for the cores and for the memory of four chunks."""
    edge = np.array([0, 1, 2, 100, 101, 0x7FFE, CLAMP], np.uint32)
    rng = np.random.default_rng(21)
    n = 4096
    free = rng.choice(edge, size=(n, 4, 2))
    req = rng.choice(edge, size=(n, 2))
    grid = np.array(list(itertools.product(edge, repeat=4)), np.uint32)  # (free c, free m, request c, request m)
    free = np.concatenate([free, np.broadcast_to(grid[:, None, :2], (len(grid), 4, 2))])
    req = np.concatenate([req, grid[:, 2:]])
    free[n:, 1:, :] = rng.choice(edge, size=(len(grid), 3, 2))  # (the other chunks vary beside chunk 0)
    node = [(free[:, c, 0] + np.uint32(GUARD)) | ((free[:, c, 1] + np.uint32(GUARD)) << np.uint32(16)) for c in range(4)]
    rq = req[:, 0] | (req[:, 1] << np.uint32(16))
    d = [pk_sub_u16(node[c], rq) for c in range(4)]
    fits_c = [(free[:, c, 0] >= req[:, 0]).astype(np.uint32) for c in range(4)]
    fits_m = [(free[:, c, 1] >= req[:, 1]).astype(np.uint32) for c in range(4)]
    want = expected(fits_c, fits_m)
    np.testing.assert_array_equal(mask_perm_then_and(d), want)
    np.testing.assert_array_equal(mask_and_then_perm(d), want)
    at_clamp = (req == CLAMP).any(axis=1)
    assert at_clamp.sum() > 500 and want[at_clamp].any() and (want[at_clamp] == 0).any()


def test_a_wrong_selector_pairs_other_chunks():
    """The model tells the selectors apart: with the gathering selector in front of the ANDs, chunk 0's cores
    guard meets chunk 0's memory guard in the wrong half, and the mask differs for some combination."""
    d, cb, mb = guard_combinations(junk=2)
    want = expected(cb, mb)
    assert (mask_perm_then_and(d, SEL_GATHER) != want).any()
    for sel in (0x0B0A0908, 0x0A0B0908, 0x0B09080A, 0x090B080A):
        assert (mask_perm_then_and(d, sel) != want).any(), hex(sel)
