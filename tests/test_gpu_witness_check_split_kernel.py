"""gpu tier: tkmk_witness_check_copy_split (csrc/witcheck.hip), the copy comparison of one rank of a sharded prover — this rank's cells
against a buffer of gathered source values — against numpy and Python integers mod r.  One lane per entry, 64 lanes a wave, four waves
a workgroup: the entry counts sit on both sides of a wave (63, 64, 65) and of a workgroup (255, 256, 257) and reach a fourth workgroup
(1000); the single failures sit on the same edges.  Both results are a count and a minimum over integers, so every call is made twice
and must repeat itself.  The two buffers are exactly local_cells / n_sources elements long and the out-of-range entries point at the
first element behind them: the assertions are on the return code and the counts."""
import random

import numpy as np
import pytest

from pyref import R

pytestmark = pytest.mark.gpu
COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 1000]
LOCAL_CELLS, N_SOURCES = 37, 53          # neither a multiple of anything the kernel tiles by


def _bytes(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), np.uint8)


class Split:
    """b_local and sources drawn from a pool of four residues (so that equal and unequal pairs are both plentiful), some of them stored
    as v + r: the second representation of the residue v that fits 256 bits"""

    def __init__(self, tk, seed):
        rnd = random.Random(seed)
        pool = [rnd.randrange(R) for _ in range(3)] + [0]
        self.tk, self.rnd = tk, rnd
        self.b = [rnd.choice(pool) for _ in range(LOCAL_CELLS)]
        self.src = [rnd.choice(pool) for _ in range(N_SOURCES)]
        for vals in (self.b, self.src):                                    # every third element in its other representation where that fits
            for k in range(0, len(vals), 3):
                if vals[k] + R < 1 << 256:
                    vals[k] += R
        assert any(v >= R for v in self.b) and any(v >= R for v in self.src) and any(v < R for v in self.b)
        self.d_b, self.d_src = tk.DeviceBuffer.from_host(_bytes(self.b)), tk.DeviceBuffer.from_host(_bytes(self.src))
        pairs = [(d, s) for d in range(LOCAL_CELLS) for s in range(N_SOURCES)]
        self.equal = [p for p in pairs if (self.b[p[0]] - self.src[p[1]]) % R == 0]
        self.differ = [p for p in pairs if (self.b[p[0]] - self.src[p[1]]) % R != 0]
        # the pool makes pairs equal as residues whose stored integers differ: the comparison must be on residues
        assert any(self.b[d] != self.src[s] for d, s in self.equal)

    def good(self, n):
        return [self.rnd.choice(self.equal) for _ in range(n)]

    def wrong(self):
        return self.rnd.choice(self.differ)

    def run(self, entries):
        """-> the kernel's (bad, first, in_range), after it agreed with the integers and with its own second run"""
        tk = self.tk
        dst, slot = [e[0] for e in entries], [e[1] for e in entries]
        got = tk.witness_check_copy_split(self.d_b, LOCAL_CELLS, dst, self.d_src, N_SOURCES, slot)
        assert got == tk.witness_check_copy_split(self.d_b, LOCAL_CELLS, dst, self.d_src, N_SOURCES, slot)
        inside = [d < LOCAL_CELLS and s < N_SOURCES for d, s in entries]
        bad = [k for k, (d, s) in enumerate(entries) if inside[k] and (self.b[d] - self.src[s]) % R != 0]
        assert got == (len(bad), bad[0] if bad else None, all(inside)), (got, bad[:4], all(inside))
        return got


@pytest.fixture(scope="module")
def split(gpu):
    return Split(gpu, seed=31)


@pytest.mark.parametrize("n", COUNTS)
def test_no_entry_fails(split, n):
    assert split.run(split.good(n)) == (0, None, True)


def test_zero_entries_need_no_buffers(gpu):
    assert gpu.witness_check_copy_split(None, 0, [], None, 0, []) == (0, None, True)


@pytest.mark.parametrize("n", [c for c in COUNTS if c])
def test_every_entry_fails(split, n):
    assert split.run([split.wrong() for _ in range(n)]) == (n, 0, True)


@pytest.mark.parametrize("n", [c for c in COUNTS if c])
def test_one_failing_entry_on_the_wave_and_workgroup_edges(split, n):
    for at in sorted({0, n - 1} | {k for k in (63, 64, 256) if k < n}):
        entries = split.good(n)
        entries[at] = split.wrong()
        assert split.run(entries) == (1, at, True), (n, at)


def test_restarting_behind_a_hit_walks_all_failures_in_order(gpu, split):
    n = 1000
    entries = split.good(n)
    failing = [0, 1, 63, 64, 65, 255, 256, 257, 600, 999]
    for k in failing:
        entries[k] = split.wrong()
    dst = gpu.DeviceBuffer.from_host(np.array([e[0] for e in entries], np.uint32).view(np.uint8))
    slot = gpu.DeviceBuffer.from_host(np.array([e[1] for e in entries], np.uint32).view(np.uint8))

    class View:                                        # the arrays from entry `start` on, as host/tkmk_witness_check.hpp restarts
        def __init__(self, buf, start):
            self.ptr, self.nbytes = buf.ptr + 4 * start, buf.nbytes - 4 * start
    walked, start = [], 0
    while start < n:
        bad, first, in_range = gpu.witness_check_copy_split(split.d_b, LOCAL_CELLS, View(dst, start), split.d_src, N_SOURCES, View(slot, start))
        assert in_range and bad == len(failing) - len(walked)
        if first is None:
            break
        walked.append(start + first)
        start += first + 1
    assert walked == failing


def test_two_representations_of_one_residue_are_equal(gpu):
    """v against v + r, both ways round, for the residues at the ends of the range in which v + r still fits 256 bits"""
    top = (1 << 256) - 1 - R
    vals = [0, 1, 2, top - 1, top, R - 1 if R - 1 <= top else top]
    b = vals + [v + R for v in vals]
    src = [v + R for v in vals] + vals
    d_b, d_src = gpu.DeviceBuffer.from_host(_bytes(b)), gpu.DeviceBuffer.from_host(_bytes(src))
    n = len(b)
    assert gpu.witness_check_copy_split(d_b, n, list(range(n)), d_src, n, list(range(n))) == (0, None, True)
    # ... and the neighbouring residue is not: every entry against the next value's slot
    shifted = [(k + 1) % len(vals) + (len(vals) if k >= len(vals) else 0) for k in range(n)]
    want = [k for k in range(n) if (b[k] - src[shifted[k]]) % R != 0]
    assert len(want) == n
    assert gpu.witness_check_copy_split(d_b, n, list(range(n)), d_src, n, shifted) == (n, 0, True)


@pytest.mark.parametrize("which", ["dst", "slot", "both"])
def test_an_entry_outside_its_buffer_is_skipped_and_reported(split, which):
    """code 11 (in_range False) with every other entry judged; the offending index is the first element BEHIND a buffer of exactly
    local_cells / n_sources elements, and far behind it"""
    good = split.good(300)
    wrong = split.wrong()
    for d_out, s_out in ((LOCAL_CELLS, N_SOURCES), (0xFFFFFFFF, 0xFFFFFFFF)):
        outside = {"dst": (d_out, good[0][1]), "slot": (good[0][0], s_out), "both": (d_out, s_out)}[which]
        entries = good[:100] + [outside] + good[101:280] + [wrong] + good[281:]
        assert split.run(entries) == (1, 280, False)
        assert split.run([outside] + good[1:]) == (0, None, False)
        assert split.run([outside] * 70) == (0, None, False)


def test_repeated_and_descending_slots(split):
    n = 257
    by_slot = {}
    for d, s in split.equal:
        by_slot.setdefault(s, []).append(d)
    s0 = max(by_slot, key=lambda s: len(by_slot[s]))
    repeated = [(split.rnd.choice(by_slot[s0]), s0) for _ in range(n)]          # one slot for every entry
    assert split.run(repeated) == (0, None, True)
    repeated[200] = next(p for p in split.differ if p[1] == s0)
    assert split.run(repeated) == (1, 200, True)
    descending = []                                                               # slots N_SOURCES - 1 .. 0, again and again
    for k in range(n):
        s = N_SOURCES - 1 - k % N_SOURCES
        descending.append((split.rnd.choice(by_slot[s]), s) if s in by_slot else None)
    descending = [p for p in descending if p is not None]
    assert len(descending) > 200 and any(a[1] > b[1] for a, b in zip(descending, descending[1:]))
    assert split.run(descending) == (0, None, True)
    descending[64] = next(p for p in split.differ if p[1] == descending[64][1])
    assert split.run(descending) == (1, 64, True)
