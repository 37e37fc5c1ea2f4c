"""not-gpu tier: witness_check::merge of host/tkmk_witness_check.hpp — the one place where the blocks of G ranks (one block when there is
one rank) become the report — through tests/host_cpp/witness_merge_driver, which touches no device.  A made-up outcome of the three
sections (which placements, entries and public wires fail, with which values) is dealt to G = 1, 2, 4 ranks the way the sections own
them — placement q and the entries of column c on rank q mod G, c mod G, every rank keeping the first eight of its own — and the
merged report must be the one Python makes from the outcome as a whole, whatever G."""
import hashlib
import json
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
DRIVER = os.path.join(HERE, "host_cpp", "witness_merge_driver")
MAX_FINDINGS = 8
S_MAX, M_I = 64, 4
KINDS = [(7, "alpha"), (9, "bufferPubOut"), (11, "gamma")]
P = 40
LAYOUT = [q % len(KINDS) for q in range(P)]
WORLDS = [1, 2, 4]


def _fr(*tag):
    return int.from_bytes(hashlib.sha256(repr(tag).encode()).digest(), "big")


def _hex(v):
    return "%064x" % v


def _permutation(bijective=True):
    """100 distinct cells spread over all columns, cell k copying cell k + 1 (a cycle); not bijective: entry 6 copies entry 5's source"""
    cells = [(k % M_I, (7 * k + k // S_MAX) % S_MAX) for k in range(100)]
    assert len(set(cells)) == len(cells)
    perm = [(r, c) + cells[(k + 1) % len(cells)] for k, (r, c) in enumerate(cells)]
    if not bijective:
        perm[6] = perm[6][:2] + perm[5][2:]
    return perm


class Outcome:
    """what the three sections found, over all ranks; clean: nothing"""

    def __init__(self, clean=False, bijective=True):
        self.perm = _permutation(bijective)
        self.arithmetic = {} if clean else {q: (3 + q, 1 + q % 5, _fr("u", q), _fr("v", q), _fr("w", q)) for q in range(P)}   # every placement fails
        self.copy = {} if clean else {e: (_fr("value", e), _fr("source", e)) for e in range(len(self.perm)) if e % 3 != 1}
        self.wires = {q: 20 + q for q in range(4)}
        self.public = [] if clean else [(q, w, 5 * q + w, _fr("pub", q, w), _fr("inst", q, w)) for q in range(4) for w in range(2, 22, 2)]   # ten per placement

    def blocks(self, world, failed=None):
        """the description's lines of every rank's block; failed: {rank: (placement, text)}"""
        lines = []
        for rank in range(world):
            ar = [(q,) + self.arithmetic[q] for q in sorted(self.arithmetic) if q % world == rank]
            co = [(e,) + self.copy[e] for e in sorted(self.copy) if self.perm[e][1] % world == rank]
            pu = [f for f in sorted(self.public) if f[0] % world == rank]
            if world > 1 and ar and not failed:
                assert len(ar) >= MAX_FINDINGS and len(co) >= MAX_FINDINGS and len(pu) >= MAX_FINDINGS     # the cut after the sort matters
            fail = (failed or {}).get(rank)
            lines.append(" ".join(str(v) for v in [sum(f[2] for f in ar), len(ar), min(len(ar), MAX_FINDINGS), len(co), min(len(co), MAX_FINDINGS),
                                                   sum(n for q, n in self.wires.items() if q % world == rank), len(pu), min(len(pu), MAX_FINDINGS),
                                                   1 if fail else 0, fail[0] if fail else 0, fail[1].encode().hex() if fail else "-"]))
            lines += ["%d %d %d %s %s %s" % (f[:3] + tuple(_hex(v) for v in f[3:])) for f in ar[:MAX_FINDINGS]]
            lines += ["%d %s %s" % (f[0], _hex(f[1]), _hex(f[2])) for f in co[:MAX_FINDINGS]]
            lines += ["%d %d %d %s %s" % (f[2], f[0], f[1], _hex(f[3]), _hex(f[4])) for f in pu[:MAX_FINDINGS]]
        return lines

    def report(self):
        """the report of the whole outcome: no ranks, no blocks"""
        ar = [{"placement": q, "subcircuitId": KINDS[LAYOUT[q]][0], "name": KINDS[LAYOUT[q]][1], "first_row": f[0], "bad_rows": f[1],
               "u": "0x" + _hex(f[2]), "v": "0x" + _hex(f[3]), "w": "0x" + _hex(f[4])} for q, f in sorted(self.arithmetic.items())]
        co = [{"entry": e, "row": self.perm[e][0], "col": self.perm[e][1], "X": self.perm[e][2], "Y": self.perm[e][3], "value": "0x" + _hex(f[0]),
               "source": "0x" + _hex(f[1])} for e, f in sorted(self.copy.items())]
        pu = [{"index": f[2], "placement": f[0], "wire": f[1], "value": "0x" + _hex(f[3]), "instance": "0x" + _hex(f[4])} for f in sorted(self.public)]
        written, seen, twice = {(r, c) for r, c, _, _ in self.perm}, set(), None
        for _, _, x, y in self.perm:                    # the first source that is no destination, or is some other entry's source already
            if (x, y) not in written or (x, y) in seen:
                twice = (x, y)
                break
            seen.add((x, y))
        copy = {"ok": twice is None and not co, "entries": len(self.perm), "bijection": twice is None, "bad_entries": len(co), "first": co[:MAX_FINDINGS]}
        if twice:
            copy["hit_twice"] = {"row": twice[0], "col": twice[1]}
        reason = ""
        if ar:
            reason = ("arithmetic: placement %d (subcircuit %d, %s) does not satisfy its R1CS: %d failing row(s), the first is row %d"
                      % (0, KINDS[LAYOUT[0]][0], KINDS[LAYOUT[0]][1], ar[0]["bad_rows"], ar[0]["first_row"]))
        elif twice:
            reason = "copy: the permutation is not a bijection: cell (row %d, col %d) is the image of two cells" % twice
        return {"ok": not (ar or co or pu or twice), "reason": reason,
                "arithmetic": {"ok": not ar, "placements": P, "bad_placements": len(ar), "bad_cells": sum(f["bad_rows"] for f in ar), "first": ar[:MAX_FINDINGS]},
                "copy": copy, "public": {"ok": not pu, "wires": sum(self.wires.values()), "bad": len(pu), "first": pu[:MAX_FINDINGS]}}


def _merge(outcome, block_lines, world):
    head = ["%d %d" % (S_MAX, M_I), str(len(KINDS))] + ["%d %s" % k for k in KINDS] + [str(P), " ".join(map(str, LAYOUT)), str(len(outcome.perm))]
    text = "\n".join(head + ["%d %d %d %d" % e for e in outcome.perm] + [str(world)] + block_lines) + "\n"
    r = subprocess.run([DRIVER], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode in (0, 1), (r.returncode, r.stderr[-2000:])
    return r.returncode, r.stdout.strip()


def _report(stdout):
    doc = json.loads(stdout)
    assert set(doc.pop("seconds")) == {"parse", "upload", "build", "check", "total"}
    return doc


@pytest.mark.parametrize("world", WORLDS)
def test_findings_dealt_to_the_ranks_merge_into_the_report_of_the_whole(world):
    """every rank holds eight findings per section (G > 1), so the sort and the cut to eight decide the result; totals sum across ranks;
    a copy finding's row / col / X / Y come from the replicated permutation"""
    outcome = Outcome()
    code, out = _merge(outcome, outcome.blocks(world), world)
    assert code == 0, out
    want = outcome.report()
    assert want["arithmetic"]["bad_placements"] == P and want["copy"]["bad_entries"] > 4 * MAX_FINDINGS and want["public"]["bad"] == 40
    assert _report(out) == want


def test_every_world_size_gives_the_same_bytes():
    outcome = Outcome()
    outs = {_merge(outcome, outcome.blocks(world), world) for world in WORLDS}
    assert len(outs) == 1 and next(iter(outs))[0] == 0


@pytest.mark.parametrize("world", WORLDS)
def test_a_clean_witness(world):
    outcome = Outcome(clean=True)
    code, out = _merge(outcome, outcome.blocks(world), world)
    assert code == 0 and _report(out) == outcome.report() and _report(out)["ok"] is True and _report(out)["reason"] == ""


@pytest.mark.parametrize("world", WORLDS)
def test_a_permutation_that_is_no_bijection_fails_the_copy_section_alone(world):
    outcome = Outcome(clean=True, bijective=False)
    code, out = _merge(outcome, outcome.blocks(world), world)
    got, want = _report(out), outcome.report()
    assert code == 0 and got == want
    x, y = outcome.perm[5][2:]
    assert got["copy"] == {"ok": False, "entries": 100, "bijection": False, "hit_twice": {"row": x, "col": y}, "bad_entries": 0, "first": []}
    assert got["ok"] is False and got["arithmetic"]["ok"] and got["public"]["ok"] and got["reason"].startswith("copy: the permutation is not a bijection")


def test_the_input_error_of_the_lowest_placement_is_the_error():
    """ranks 3 and 1 of four both saw one, in placements 3 and 1: the text of placement 1 leaves, whatever the rank order"""
    outcome = Outcome()
    failed = {3: (3, "instance.json: no value for public wire 77"), 1: (1, "subcircuitInfo.json: public wire mapped outside [0, l)")}
    assert _merge(outcome, outcome.blocks(4, failed), 4) == (1, "error: " + failed[1][1])
    swapped = {1: (3, failed[3][1]), 3: (1, failed[1][1])}
    assert _merge(outcome, outcome.blocks(4, swapped), 4) == (1, "error: " + failed[1][1])
    full = "x" * 248                                       # a text that fills the block's field: no terminator inside it
    assert _merge(outcome, outcome.blocks(2, {0: (0, full)}), 2) == (1, "error: " + full)


@pytest.mark.parametrize("world", WORLDS)
def test_a_block_that_claims_nine_findings_is_malformed(world):
    outcome = Outcome()
    lines = outcome.blocks(world)
    first = lines[0].split()
    assert first[4] == str(MAX_FINDINGS)
    first[4] = "9"                                         # n_copy
    assert _merge(outcome, [" ".join(first)] + lines[1:], world) == (1, "error: witness check: a rank's block is malformed: unknown error")   # TKMK_ERR_UNKNOWN's text is appended
