#!/usr/bin/env python3
"""Write tests/golden/fe_*.npz from the reference findErrors.

    tools/make_fe_golden.py [--findErrors PATH] [--out tests/golden]

The binary is oracle/_ref/fe_ref, which `make -C oracle` compiles from the reference sources
where they lie ("Reference binary for findErrors"); nothing of it is committed.  Reads and overlaps come from
fixed seeds; the gkpStore is written by the reference's own gkStore code
(oracle.build_gkpstore), the overlap store by its own ovStore writer (oracle.build_store), and
the command line is canu's (OverlapErrorAdjustment.pm:194-202).  Fixtures e..i are the
constructed vote cases of tests/fe_votes.py, one option line each.  Each fixture holds the reads,
the store's records of the range (what Read_Olaps loads), the reference's .red bytes, its
passed / failed counts, the range and the options.
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fe_restate as FR  # noqa: E402
import fe_votes as FV  # noqa: E402

_ACGT = b"ACGT"
_COMP = bytes.maketrans(b"ACGTN", b"TGCAN")


def _rc(b: bytes) -> bytes:
    return b.translate(_COMP)[::-1]


def _rand(rng, n: int) -> bytes:
    return np.frombuffer(_ACGT, dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()


def _mutate(rng, seg: bytes, err: float):
    """Substitutions, insertions and deletions, a third each -> (read, pos) where pos[i] is
    the read offset of segment base i (of the next kept base for a deleted one)."""
    out = bytearray()
    pos = np.zeros(len(seg) + 1, dtype=np.int64)
    for i, c in enumerate(seg):
        pos[i] = len(out)
        u = rng.random()
        if u < err / 3:
            out.append(_ACGT[(_ACGT.index(c) + int(rng.integers(1, 4))) % 4])
        elif u < 2 * err / 3:
            out.append(c)
            out.append(_ACGT[int(rng.integers(0, 4))])
        elif u < err:
            continue
        else:
            out.append(c)
    pos[len(seg)] = len(out)
    return bytes(out), pos


class Sample:
    """Reads cut from one genome, with where every genome base went."""

    def __init__(self, seed: int, genome_len: int, n_reads: int, err: float,
                 lo: int = 1500, hi: int = 3000):
        self.rng = rng = np.random.default_rng(seed)
        self.genome = _rand(rng, genome_len)
        self.reads: list[bytes] = []
        self.where: list = []                     # genome start, end, strand, pos map
        for _ in range(n_reads):
            L = int(rng.integers(lo, hi + 1))
            s = int(rng.integers(0, genome_len - L + 1))
            self.add(s, s + L, int(rng.integers(0, 2)), err)

    def add(self, s: int, e: int, strand: int, err: float) -> int:
        r, pos = _mutate(self.rng, self.genome[s:e], err)
        self.reads.append(_rc(r) if strand else r)
        self.where.append((s, e, strand, pos))
        return len(self.reads)

    def add_raw(self, seq: bytes) -> int:
        self.reads.append(seq)
        self.where.append((-1, -1, 0, None))
        return len(self.reads)

    def record(self, a: int, b: int, min_true: int = 500, jitter: int = 0):
        """The overlap of reads a, b (IDs) with the hangs the genome gives, in read offsets."""
        sa, ea, ta, pa = self.where[a - 1]
        sb, eb, tb, pb = self.where[b - 1]
        lo, hi = max(sa, sb), min(ea, eb)
        if sa < 0 or sb < 0 or hi - lo < min_true:
            return None
        alen, blen = len(self.reads[a - 1]), len(self.reads[b - 1])
        a_lo, a_hi = int(pa[lo - sa]), int(pa[hi - sa])
        b_lo, b_hi = int(pb[lo - sb]), int(pb[hi - sb])
        if ta == 0:
            a_hang, b_hang = a_lo - b_lo, (blen - b_hi) - (alen - a_hi)
        else:
            a_hang, b_hang = (alen - a_hi) - (blen - b_hi), b_lo - a_lo
        if jitter:
            a_hang += int(self.rng.integers(-jitter, jitter + 1))
        a_hang = min(max(a_hang, -(blen - 1)), alen - 1)
        return FR.make_record(a, b, a_hang, b_hang, ta != tb)

    def all_pairs(self, limit: int, jitter: int = 0):
        recs = []
        n = len(self.reads)
        for a in range(1, n + 1):
            for b in range(a + 1, n + 1):
                r = self.record(a, b, jitter=jitter if (a + b) % 5 == 0 else 0)
                if r is not None:
                    recs.append(r)
        self.rng.shuffle(recs)
        return recs[:limit]


def false_pairs(S: Sample, recs: list, k: int):
    """Overlaps the reads do not have."""
    n, got = len(S.reads), 0
    for a in range(1, n + 1):
        for b in range(n, a, -1):
            if got < k and S.where[a - 1][0] >= 0 and S.record(a, b, min_true=1) is None:
                recs.append(FR.make_record(a, b, 150 * (1 if got % 2 else -1), 100, got % 3 == 0))
                got += 1


def island(S: Sample, recs: list, flip_all: bool = False, haplo: bool = False):
    """A read of its own sequence with one planted difference of every vote type, and seven
    reads that agree against it: at four places an inserted base (3 + 2 + 2 votes over three
    letters -- the reference writes an insert only when 2 * max < total, and looks at the inserts
    of a base only when it is confirmed twice or has a substitution record, so that only
    end_exclude_len 0 shows them here), four substitutions
    (one to each letter), a deletion.  With `haplo`, one more place where three of the seven
    say one letter and four another."""
    rng = S.rng
    truth = bytearray(_rand(rng, 900))
    ins_at = [120, 200, 280, 360]
    for k, p in enumerate(ins_at):
        truth[p] = truth[p + 1] = _ACGT[(k + 1) % 4]      # the inserted letters all differ
    a_read = bytearray(truth)
    sub_at = [440, 500, 560, 620]
    for k, p in enumerate(sub_at):                          # A is wrong; the truth is letter k
        truth[p] = _ACGT[k]
        a_read[p] = _ACGT[(k + 1) % 4]
    del_at = 700
    hap_at = 780
    a = S.add_raw(bytes(a_read[:del_at]) + bytes([_ACGT[(_ACGT.index(truth[del_at]) + 2) % 4]])
                  + bytes(a_read[del_at:]))
    for r in range(7):
        b = bytearray(truth)
        if haplo:
            b[hap_at] = _ACGT[(_ACGT.index(a_read[hap_at]) + (1 if r < 3 else 2)) % 4]
        for k, p in reversed(list(enumerate(ins_at))):
            others = [c for c in range(4) if c != (k + 1) % 4 and c != k]
            letter = k if r < 3 else others[0] if r < 5 else others[1]
            b[p + 1:p + 1] = bytes([_ACGT[letter]])
        flipped = flip_all or r % 2 == 1
        bid = S.add_raw(_rc(bytes(b)) if flipped else bytes(b))
        recs.append(FR.make_record(a, bid, 0, len(b) - (len(a_read) + 1), flipped))
    return a


def fixture_a():
    S = Sample(5101, 24000, 70, 0.012)
    recs = S.all_pairs(320, jitter=60)
    false_pairs(S, recs, 6)
    island(S, recs)
    return S.reads, recs, 4, len(S.reads) - 3, ["-e", "0.045"]


def fixture_b():
    S = Sample(5102, 16000, 44, 0.08, lo=1200, hi=2400)
    recs = S.all_pairs(220, jitter=80)
    false_pairs(S, recs, 6)
    island(S, recs, flip_all=True)
    return S.reads, recs, 1, len(S.reads), ["-e", "0.144", "-k", "8", "-V", "6", "-x", "0"]


def fixture_c():
    S = Sample(5103, 16000, 44, 0.02, lo=1200, hi=2400)
    recs = S.all_pairs(200, jitter=60)
    false_pairs(S, recs, 6)
    island(S, recs, haplo=True)
    return S.reads, recs, 3, len(S.reads), ["-e", "0.06", "-p", "-d", "4"]


def fixture_d():
    """The edge set; every kind once with B forward and once with B flipped."""
    S = Sample(5104, 12000, 16, 0.01, lo=800, hi=1600)
    rng = S.rng
    recs = S.all_pairs(40)
    G = S.genome
    first_edge = len(S.reads) + 1
    lonely = S.add_raw(_rand(rng, 700))                     # in range, no overlaps
    for fl in (0, 1):
        o = (lambda s: _rc(s)) if fl else (lambda s: s)
        # exact matches: dovetail (a_hang > 0), a_hang < 0, a_hang == 0, contained both ways
        a = S.add_raw(G[1000:2200])
        b = S.add_raw(o(G[1500:2700]))
        recs.append(FR.make_record(a, b, 500, 500, fl))
        c = S.add_raw(o(G[700:1900]))
        recs.append(FR.make_record(a, c, -300, -300, fl))
        d = S.add_raw(o(G[1000:2500]))
        recs.append(FR.make_record(a, d, 0, 300, fl))
        e = S.add_raw(o(G[1200:1800]))
        recs.append(FR.make_record(a, e, 200, -400, fl))
        # unrelated reads
        u = S.add_raw(_rand(rng, 900))
        v = S.add_raw(_rand(rng, 1000))
        recs.append(FR.make_record(u, v, 300, 400, fl))
        recs.append(FR.make_record(u, a, 0, 300, fl))
        # B leaves A in the middle of the overlap: fails
        a2 = S.add_raw(G[3000:4400])
        b2 = S.add_raw(o(G[3400:3900] + _rand(rng, 900)))
        recs.append(FR.make_record(a2, b2, 400, 400, fl))
        # B leaves A in A's last base after using up every allowed error: rescued
        L = 1000
        arr = bytearray(G[5000:5000 + L])
        barr = bytearray(arr) + bytearray(G[5000 + L:5400 + L])
        for p in np.linspace(30, L - 40, 60).astype(int):
            barr[p] = _ACGT[(_ACGT.index(barr[p]) + 1) % 4]
        barr[L - 1] = _ACGT[(_ACGT.index(barr[L - 1]) + 1) % 4]
        a3 = S.add_raw(G[4600:5000] + bytes(arr))
        b3 = S.add_raw(o(bytes(barr)))
        recs.append(FR.make_record(a3, b3, 400, 400, fl))
        # bytes that are not ACGT, on both sides
        ra = bytearray(G[6000:7200])
        rb = bytearray(G[6400:7600])
        ra[700:712] = b"N" * 12
        ra[33:34] = b"N"
        rb[500:520] = b"N" * 20
        rb[1100:1101] = b"N"
        a4 = S.add_raw(bytes(ra))
        b4 = S.add_raw(o(bytes(rb)))
        recs.append(FR.make_record(a4, b4, 400, 400, fl))
        # the same pair in both orientations
        recs.append(FR.make_record(a4, b, 100, 100, 1 - fl))
        # a homopolymer
        h1 = S.add_raw(b"A" * 600)
        h2 = S.add_raw((b"T" if fl else b"A") * 700)
        recs.append(FR.make_record(h1, h2, 200, 300, fl))
        recs.append(FR.make_record(h1, h2, -50, 50, fl))
    island(S, recs)
    last_in_range = len(S.reads)
    # more than 255 copies of one stretch of a read, each with the same one difference
    base = bytearray(G[8000:9000])
    deep = S.add_raw(bytes(base))
    last_in_range = deep
    piece = bytearray(base[20:240])
    piece[100] = _ACGT[(_ACGT.index(piece[100]) + 1) % 4]
    for r in range(300):
        fl = r % 2
        c = S.add_raw(_rc(bytes(piece)) if fl else bytes(piece))    # B reads outside the range
        recs.append(FR.make_record(deep, c, 20, -(1000 - 240), fl))   # :282 lets only early changes vote
    assert lonely >= first_edge
    return S.reads, recs, 3, last_in_range, ["-e", "0.06"]


def lab_fixture(name: str):
    """Fixtures e..i: the constructed vote cases of tests/fe_votes.py, one option line each."""
    def mk():
        lab = FV.fixture(name)
        FV.restate(lab)                       # every site carries the tally it was built for
        reads, recs, bgn, end = lab.job()
        return reads, recs, bgn, end, lab.args
    return mk


FIXTURES = [("a", fixture_a), ("b", fixture_b), ("c", fixture_c), ("d", fixture_d)] + \
    [(n, lab_fixture(n)) for n in "efghi"]


def lab_assertions(name: str, red) -> None:
    """What each of e..i is there for, counted on the reference's own records."""
    t = (red["word"] >> 2) & 15
    pos = red["word"] >> 6
    rec = red[t != 0]
    key = rec["readID"].astype(np.uint64) << np.uint64(32) | (rec["word"] >> 6)
    _, n = np.unique(key, return_counts=True)
    two = int((n == 2).sum())                              # bases with two records
    ins = int((t >= FR.A_INSERT).sum())
    at = set(int(v) for v in pos[t != 0])
    assert at >= {254, 255, 256, 257, 511, 512}, (name, sorted(at))
    keep = red["word"][t == 0] & 3
    assert set(int(v) for v in keep) == {0, 1, 2, 3}, (name, "degrees on both sides of -d")
    if name in "eh":        # no insert record is possible: the haplotype count refuses them
        assert ins == 0 and two == 0 and (t == FR.DELETE).any(), (name, ins, two)
    if name == "f":         # substitution + insert and delete + insert at one base
        assert two >= 10 and ins == two, (name, ins, two)
        d = rec[(rec["word"] >> 2) & 15 == FR.DELETE]
        dk = set((int(r["readID"]), int(r["word"]) >> 6) for r in d)
        ik = set((int(r["readID"]), int(r["word"]) >> 6) for r in rec
                 if (int(r["word"]) >> 2) & 15 >= FR.A_INSERT)
        assert len(dk & ik) >= 2, (name, "delete and insert records at one base")
    if name in "gi":        # inserts through `confirmed`, never next to another record
        assert ins >= 5 and two == 0, (name, ins, two)
    if name == "i":
        assert ins > 5, name


def read_set(reads: list[bytes]):
    from canu_amd.synth import ReadSet
    lens = np.array([len(r) for r in reads], dtype=np.uint32)
    offs = np.zeros(len(reads), dtype=np.uint64)
    if len(reads) > 1:
        offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    return ReadSet(bases=np.frombuffer(b"".join(reads), dtype=np.uint8).copy(), offsets=offs,
                   lengths=lens, first_iid=1)


def run_reference(binary, reads, recs, bgn, end, args):
    import oracle
    from canu_amd.overlap_in_core import RECORD_DTYPE
    rs = read_set(reads)
    raw, passed, failed, sel = oracle.run_find_errors(rs, np.array(recs, dtype=RECORD_DTYPE),
                                                      bgn, end, args, binary=binary)
    return rs, sel, raw, passed, failed


def store_fixture(out_dir: str) -> None:
    """tests/golden/fe_store.npz: the bytes of a small store the reference wrote, its content as
    the reference's ovStore reader dumps it, and two -R ranges of it."""
    import oracle
    from canu_amd.overlap_in_core import RECORD_DTYPE, write_ovb
    S = Sample(5105, 8000, 40, 0.01, lo=600, hi=1200)
    recs = [r for r in S.all_pairs(120) if r[0] not in (1, 7) and r[1] not in (1, 7)]
    rs = read_set(S.reads)
    inp = np.array(recs, dtype=RECORD_DTYPE)
    with tempfile.TemporaryDirectory() as d:
        gkp = oracle.build_gkpstore(rs, d)
        ovb = os.path.join(d, "in.ovb")
        write_ovb(inp, ovb, counts=False)
        store = os.path.join(d, "asm.ovlStore")
        oracle.build_store(gkp, store, [ovb])
        stored = oracle.dump_store(gkp, store)
        files = sorted(os.listdir(store))
        blobs = {f: np.frombuffer(open(os.path.join(store, f), "rb").read(), dtype=np.uint8)
                 for f in files}
    assert "info" in blobs and "index" in blobs and "0001" in blobs, files
    ranges = np.array([[3, 9], [1, len(S.reads)]], dtype=np.uint32)
    path = os.path.join(out_dir, "fe_store.npz")
    np.savez_compressed(path, names=np.array(files), ranges=ranges,
                        **{"file_" + f: b for f, b in blobs.items()},
                        **{"rec_" + f: stored[f] for f in stored.dtype.names})
    print(path, os.path.getsize(path), "bytes;", stored.shape[0], "overlaps; files", files)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--findErrors", default=os.path.join(ROOT, "oracle", "_ref", "fe_ref"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    types = set()
    for name, mk in FIXTURES:
        reads, recs, bgn, end, args = mk()
        rs, sel, raw, passed, failed = run_reference(os.path.abspath(a.findErrors), reads, recs,
                                                     bgn, end, args)
        red = np.frombuffer(raw, dtype=FR.RED_DTYPE)
        t = (red["word"] >> 2) & 15
        types |= set(int(v) for v in t)
        # the coverage this fixture is for, on what the reference produced
        assert passed > 0 and failed > 0, (name, passed, failed)
        ids, n = np.unique(red["readID"], return_counts=True)
        assert ids.shape[0] == end - bgn + 1 and (n == 1).any(), name
        if name in "efghi":
            lab_assertions(name, red)
        if name == "d":
            keep = red["word"][t == 0] & 3
            assert set(int(v) & 1 for v in keep) == {0, 1}, "keep_left takes one value"
            assert set(int(v) >> 1 for v in keep) == {0, 1}, "keep_right takes one value"
            deep = red[red["readID"] == end]
            assert ((deep["word"] >> 2) & 15 != 0).any(), "the saturated vote gave no record"
        path = os.path.join(a.out, f"fe_{name}.npz")
        np.savez_compressed(
            path, bases=rs.bases, offsets=rs.offsets, lengths=rs.lengths,
            **{"in_" + f: sel[f] for f in sel.dtype.names},
            red=np.frombuffer(raw, dtype=np.uint8),
            counters=np.array([passed, failed, bgn, end], dtype=np.uint64),
            args=np.frombuffer(" ".join(args).encode(), dtype=np.uint8))
        print(path, os.path.getsize(path), "bytes;", sel.shape[0], "overlaps;", red.shape[0],
              "records; passed", passed, "failed", failed, "types", sorted(set(int(v) for v in t)))
    assert types >= set(range(10)), f"vote types missing from the fixtures: {set(range(10)) - types}"
    store_fixture(a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
