"""findErrors on the GPU (libcanu_fe.so): the reference's .red bytes on the fixtures, and the
shapes, boundaries, error paths and constructed vote cases (tests/fe_votes.py) against the
Python restatement (tests/fe_restate.py, itself pinned to the reference by
tests/test_fe_cpu.py)."""
import os

import numpy as np
import pytest

import fe_restate as FR
import fe_votes as FV
from canu_amd import find_errors as FE
from canu_amd.overlap_in_core import RECORD_DTYPE
from canu_amd.synth import ReadSet

pytestmark = pytest.mark.gpu

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _rand(rng, n):
    return _ACGT[rng.integers(0, 4, n)].tobytes()


def _rc(b):
    return b.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]


def _mutate(rng, seg, err):
    out = bytearray()
    for c in seg:
        u = rng.random()
        if u < err / 3:
            out.append(b"ACGT"[(b"ACGT".index(c) + int(rng.integers(1, 4))) % 4])
        elif u < 2 * err / 3:
            out += bytes([c, b"ACGT"[int(rng.integers(0, 4))]])
        elif u >= err:
            out.append(c)
    return bytes(out)


def _read_set(reads):
    lens = np.array([len(r) for r in reads], dtype=np.uint32)
    offs = np.zeros(len(reads), dtype=np.uint64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    return ReadSet(bases=np.frombuffer(b"".join(reads), dtype=np.uint8).copy(), offsets=offs,
                   lengths=lens, first_iid=1)


def _params(o):
    return FE.FeParameters(o["erate"], o["degree_threshold"], o["kmer_len"],
                           o["vote_qualify_len"], o["end_exclude_len"], o["use_haplo_ct"])


def _gpu(reads, recs, bgn, end, o, env=None):
    """-> (.red records, counters, stats) of the library."""
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        fe = FE.FindErrors(_params(o))
        fe.load_reads(_read_set(reads))
        out = fe.run(np.array(recs, dtype=RECORD_DTYPE), bgn, end)
        c, s = fe.counters(), fe.stats()
        fe.close()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    return out, c, s


def _want(reads, recs, bgn, end, o):
    st = {}
    red, p, f = FR.find_errors(np.array(recs, dtype=RECORD_DTYPE),
                               {i + 1: r for i, r in enumerate(reads)}, bgn, end, o, st)
    return red, {"passed": p, "failed": f}, st


def _same(got, want):
    assert got.shape == want.shape and np.array_equal(got, want), \
        "library:\n" + FE.dump_red(got[:40]) + "restatement:\n" + FE.dump_red(want[:40])


def _check(reads, recs, bgn, end, o, env=None):
    want, wc, st = _want(reads, recs, bgn, end, o)
    got, gc, gs = _gpu(reads, recs, bgn, end, o, env)
    _same(got, want)
    assert gc == wc
    assert gs["bases"] == st["bases"]
    return gs, st


@pytest.mark.parametrize("name", FR.FIXTURES)
def test_fixture_equals_reference(built, name):
    rs, inp, red, passed, failed, bgn, end, args = FR.golden(name)
    P, _ = FE.parse_findErrors_args(["-G", "g", "-O", "o", *args])
    fe = FE.FindErrors(P)
    fe.load_reads(rs)
    got = fe.run(inp, bgn, end)
    assert got.tobytes() == red.tobytes(), FE.dump_red(got[:30]) + "\n" + FE.dump_red(red[:30])
    assert fe.counters() == {"passed": passed, "failed": failed}
    fe.close()


@pytest.mark.parametrize("L", [1, 31, 32, 33, 63, 64, 65, 2049])
def test_overlap_lengths(built, L):
    """A's last L bases over B's first L, B forward and flipped, with and without errors."""
    rng = np.random.default_rng(100 + L)
    reads, recs = [], []
    for err in (0.0, 0.05):
        for fl in (0, 1):
            x = _rand(rng, L)
            a = _rand(rng, 300) + x
            y = _mutate(rng, x, err) if L > 8 else x
            b = (y or x[:1]) + _rand(rng, 300)
            reads += [a, _rc(b) if fl else b]
            recs.append(FR.make_record(len(reads) - 1, len(reads), 300, 300, fl))
    o = FR.defaults()
    o["erate"] = 0.144
    _check(reads, recs, 1, len(reads), o)


def _periodic(n, cut):
    """A run of one letter with another letter every 16 bases, not the same one in both reads:
    every diagonal keeps pace, so the band widens by two per error."""
    a = bytearray(b"A" * n)
    b = bytearray(b"A" * n)
    for p in range(15, n, 16):
        a[p], b[p] = ord("C"), ord("G")
    return bytes(a), bytes(b)[cut:]


@pytest.mark.parametrize("n,cut,width", [(500, 0, 63), (500, 1, 64), (520, 0, 65), (1200, 0, 119)])
def test_register_window_boundary(built, n, cut, width):
    """Widest rows of FE_WINDOW_DIAGS - 1, FE_WINDOW_DIAGS and + 1 diagonals; the last leave the
    register window for the path that reads the row before from the row log."""
    a, b = _periodic(n, cut)
    o = FR.defaults()
    o["erate"] = 0.144
    recs = [FR.make_record(1, 2, 0, 0, 0), FR.make_record(2, 1, 0, 0, 0)]
    gs, st = _check([a, b], recs[:1], 1, 2, o)
    assert st["max_width"] == width                      # the restatement's own band
    assert gs["n_generic"] == (1 if width > FE.WINDOW_DIAGS else 0)
    assert gs["rows"] == st["rows"] and gs["regrows"] == 0
    _check([a, b], recs, 1, 2, o)


@pytest.mark.parametrize("side", ["a", "b"])
@pytest.mark.parametrize("span", [FE.LDS_BASES - 1, FE.LDS_BASES, FE.LDS_BASES + 1])
def test_lds_strand_capacity(built, span, side):
    """The longer reachable span of FE_LDS_BASES - 1, FE_LDS_BASES and + 1 bases (reads of
    ~8.6 kb, which this boundary needs): up to the capacity both spans are staged in LDS, past
    it on either side the alignment reads global memory.  The other read ends 100 bases short,
    less than the errors allowed, so the long span is reachable to its end.  The spans start 7
    and 5 bases into their words."""
    rng = np.random.default_rng(span)
    x = _rand(rng, span)
    y = _mutate(rng, x[:span - 100], 0.03)
    reads, recs = [], []
    for fl in (0, 1):
        if side == "a":                      # a_part is the long span, B ends inside it
            a, b, ah, bh = _rand(rng, 407) + x, y, 407, -100
        else:                                # b_part is the long span, A ends inside it
            a, b, ah, bh = y, _rand(rng, 421) + x, -421, 100
        reads += [a, _rc(b) if fl else b]
        recs.append(FR.make_record(len(reads) - 1, len(reads), ah, bh, fl))
    short = [_rand(rng, 300) + x[:900], x[:900] + _rand(rng, 200)]     # one that is staged anyway
    reads += short
    recs.append(FR.make_record(len(reads) - 1, len(reads), 300, 200, 0))
    o = FR.defaults()
    o["erate"] = 0.06
    gs, st = _check(reads, recs, 1, len(reads), o)
    assert gs["n_staged"] == (3 if span <= FE.LDS_BASES else 1)
    assert gs["rows"] == st["rows"] > 100 and gs["regrows"] == 0


@pytest.mark.parametrize("delta,regrows", [(-1, 1), (0, 0), (1, 0)])
def test_row_log_boundary_and_regrow(built, delta, regrows):
    """A first row log one entry short of what the alignment writes is an overflow: the overlap
    runs again with the worst-case log and gives the same bytes."""
    rng = np.random.default_rng(7)
    x = _rand(rng, 1500)
    reads = [x, _mutate(rng, x, 0.06), _rand(rng, 400) + x[:900], _mutate(rng, x[300:], 0.03)]
    recs = [FR.make_record(1, 2, 0, len(reads[1]) - 1500, 0)]
    o = FR.defaults()
    o["erate"] = 0.144
    _, _, st = _want(reads, recs, 1, 1, o)
    gs, _ = _check(reads, recs, 1, 1, o, {"CANU_FE_LOG_CAP": str(st["log_used"] + delta)})
    assert gs["regrows"] == regrows
    # among others that fit: only the overflowing ones run again, and nothing votes twice
    recs += [FR.make_record(1, 3, -400, -600, 0), FR.make_record(1, 4, 300, 0, 0)]
    gs, _ = _check(reads, recs, 1, 1, o, {"CANU_FE_LOG_CAP": str(st["log_used"] + delta)})
    assert gs["regrows"] == regrows
    gs, _ = _check(reads, recs, 1, 1, o, {"CANU_FE_LOG_PER_ERROR": "1"})
    assert gs["regrows"] == 1


def test_20kb_pair(built):
    rng = np.random.default_rng(20)
    x = _rand(rng, 20000)
    y = _mutate(rng, x, 0.10)
    o = FR.defaults()
    o["erate"] = 0.144
    gs, st = _check([x, y], [FR.make_record(1, 2, 0, len(y) - len(x), 0),
                             FR.make_record(2, 1, 0, len(x) - len(y), 0)], 1, 2, o)
    # both outgrow the first row log (FE_LOG_PER_ERROR entries per allowed error): one re-run
    assert gs["regrows"] == 1 and gs["n_generic"] == 2
    assert gs["rows"] > st["rows"] > 3000


def _sample(seed, n=40, err=0.02):
    rng = np.random.default_rng(seed)
    g = _rand(rng, 9000)
    reads, where, recs = [], [], []
    for _ in range(n):
        L = int(rng.integers(600, 1800))
        s = int(rng.integers(0, len(g) - L))
        fl = int(rng.integers(0, 2))
        r = _mutate(rng, g[s:s + L], err)
        reads.append(_rc(r) if fl else r)
        where.append((s, s + L, fl))
    for a in range(n):
        for b in range(n):
            (sa, ea, fa), (sb, eb, fb) = where[a], where[b]
            if a == b or min(ea, eb) - max(sa, sb) < 300:
                continue
            ah = (sb - sa) if fa == 0 else (ea - eb)
            bh = (eb - ea) if fa == 0 else (sa - sb)
            ah = min(max(ah, -(len(reads[b]) - 1)), len(reads[a]) - 1)
            recs.append(FR.make_record(a + 1, b + 1, ah, bh, fa != fb))
    return reads, recs


def test_order_independence_and_repeat(built):
    reads, recs = _sample(31)
    o = FR.defaults()
    sel = [r for r in recs if 3 <= r[0] <= len(reads) - 2]
    want, wc, _ = _want(reads, sel, 3, len(reads) - 2, o)
    first, c1, _ = _gpu(reads, sel, 3, len(reads) - 2, o)
    _same(first, want)
    assert c1 == wc and wc["passed"] > 50
    again, c2, _ = _gpu(reads, sel, 3, len(reads) - 2, o)
    rng = np.random.default_rng(1)
    shuf = [sel[i] for i in rng.permutation(len(sel))]
    other, c3, _ = _gpu(reads, shuf, 3, len(reads) - 2, o)
    assert again.tobytes() == first.tobytes() == other.tobytes() and c1 == c2 == c3


def test_saturation(built):
    """300 votes for one letter and 260 for another at one base: saturating tallies leave 255
    and 255, so 2 * max <= total and no record; counters that wrapped or did not saturate would
    give one."""
    rng = np.random.default_rng(9)
    base = _rand(rng, 600)
    p1 = bytearray(base[20:240])
    p2 = bytearray(base[20:240])
    was = b"ACGT".index(base[120])
    p1[100] = b"ACGT"[(was + 1) % 4]
    p2[100] = b"ACGT"[(was + 2) % 4]
    reads = [base] + [bytes(p1)] * 300 + [bytes(p2)] * 260
    recs = [FR.make_record(1, 2 + i, 20, -(600 - 240), 0) for i in range(560)]
    o = FR.defaults()
    o["use_haplo_ct"] = False
    got, c, _ = _gpu(reads, recs, 1, 1, o)
    want, wc, _ = _want(reads, recs, 1, 1, o)
    _same(got, want)
    assert c == wc == {"passed": 560, "failed": 0}
    assert got.shape[0] == 1                                       # the IDENT record alone
    got, _, _ = _gpu(reads, recs[:300] + recs[300:340], 1, 1, o)   # 255 against 40: a record
    assert got.shape[0] == 2 and int(got[1]["word"]) >> 6 == 120
    assert (int(got[1]["word"]) >> 2) & 15 == FR.A_SUBST + (was + 1) % 4


# ------------------------------------------------- the vote and decision ladders, by construction

def _lab_check(lab, order=None):
    """The lab's preconditions (every site carries the tally it was built for, by the
    restatement's tallies), then the library against the restatement -> the records."""
    reads, recs, bgn, end, want, p, f, _ = FV.restate(lab, order)
    _check(reads, recs, bgn, end, lab.P)
    return reads, recs, bgn, end, want


@pytest.mark.parametrize("line", sorted(FV.LINES))
@pytest.mark.parametrize("group", sorted(FV.GROUPS))
def test_vote_cases(built, group, line):
    """Each group of constructed sites under each option line (fe_votes.LINES)."""
    lab = FV.Lab(300 + ord(line), FV.LINES[line])
    FV.GROUPS[group](lab)
    lab.false_pair(0)
    _, _, _, _, want = _lab_check(lab)
    if group in ("substitution", "positions"):
        assert ((want["word"] >> 2) & 15 != 0).any()


@pytest.mark.parametrize("line", sorted(FV.LINES))
def test_positions_shuffled(built, line):
    """The votes are atomics: the overlaps in another order give the same bytes."""
    lab = FV.Lab(300 + ord(line), FV.LINES[line])
    FV.positions(lab)
    reads, recs, bgn, end, want = _lab_check(lab)
    rng = np.random.default_rng(5)
    for _ in range(2):
        order = [int(i) for i in rng.permutation(len(recs))]
        got, _, _ = _gpu(reads, [recs[i] for i in order], bgn, end, lab.P)
        assert got.tobytes() == want.tobytes()
    at = set((int(r["readID"]), int(r["word"]) >> 6) for r in want if (int(r["word"]) >> 2) & 15)
    assert set(j for _, j in at) >= set(FV.POSITIONS) | {0}


def test_short_kmer(built):
    """kmer_len < 2 * end_exclude_len: the first and third vote loops overlap and leave the run."""
    lab = FV.Lab(41, FV.LINES["h"])
    FV.short_kmer(lab)
    FV.substitution(lab)
    reads, recs, bgn, end, want, _, _, st = FV.restate(lab)
    K, X = lab.P["kmer_len"], lab.P["end_exclude_len"]
    assert set(r for r, _, _, _ in st["runs"]) >= {K, 2 * X - 1, 2 * X, 2 * X + 1}
    assert st["fs_skipped"] > 0 and any(h for _, _, _, h in st["runs"])
    _check(reads, recs, bgn, end, lab.P)


@pytest.mark.parametrize("plane,line", [
    ("subst", "f"), ("subst_confirmed_1", "e"), ("confirmed", "e"), ("insert", "i"),
    ("insert_no_insert_1", "i"), ("no_insert", "g")])
def test_vote_saturation(built, plane, line):
    """255, 256 and 300 votes on one plane, each next to counts that show whether the plane was
    held at MAX_VOTE (fe_votes.saturation)."""
    lab = FV.Lab(78, FV.LINES[line])
    for n in (255, 256, 300):
        FV.saturation(lab, plane, n)
    _lab_check(lab)


def test_insert_saturation_flips_the_decision(built):
    """300 + 200 + 60 inserted letters behind one base: 2 * 300 >= 560 would be no record; held
    at 255, 2 * 255 < 515 is one."""
    lab = FV.Lab(79, FV.LINES["i"])
    FV.insert_flip(lab)
    a, j, t = lab.want[0]
    assert t[FR.INSERT0:] == [255, 200, 60, 0]
    _, _, _, _, want = _lab_check(lab)
    assert want.shape[0] == 2 and int(want[1]["word"]) >> 6 == j
    assert (int(want[1]["word"]) >> 2) & 15 == FR.A_INSERT


@pytest.mark.parametrize("d", [1, 2, 3, 4, 13, 14, 15])
def test_degree_thresholds(built, d):
    """-d at the degree of an end and one above it, on both ends (degrees 1, 2, 3, 13, 14)."""
    lab = FV.Lab(80, FV.LINES["e"] + ["-d", str(d)])
    FV.degrees(lab)
    _, _, _, _, want = _lab_check(lab)
    assert len(set(int(w) & 3 for w in want["word"])) > 1 or d in (1, 15)


@pytest.mark.parametrize("line", sorted(FV.LINES))
def test_random_tallies(built, line):
    lab = FV.Lab(900 + ord(line), FV.LINES[line])
    FV.random_sites(lab, 20)
    _lab_check(lab)


def test_range_and_error_behaviour(built):
    rng = np.random.default_rng(3)
    reads = [_rand(rng, 500), _rand(rng, 700), _rand(rng, 300)]
    o = FR.defaults()
    got, c, _ = _gpu(reads, [], 1, 3, o)
    assert got["readID"].tolist() == [1, 2, 3] and (got["word"] == 3).all()   # IDENT, both kept
    assert c == {"passed": 0, "failed": 0}
    fe = FE.FindErrors()
    fe.load_reads(_read_set(reads))
    rec = lambda *a: np.array([FR.make_record(*a)], dtype=RECORD_DTYPE)
    for bad in (rec(3, 1, 0, 0, 0), rec(1, 4, 0, 0, 0)):           # a_iid outside, b not loaded
        with pytest.raises(FE.FeError) as e:
            fe.run(bad, 1, 2)
        assert e.value.code == -4
    for bad in (rec(1, 2, 501, 0, 0), rec(1, 3, -301, 0, 1)):      # a hang longer than its read
        with pytest.raises(FE.FeError) as e:
            fe.run(bad, 1, 3)
        assert e.value.code == -4
    with pytest.raises(FE.FeError):
        fe.run(rec(1, 2, 0, 0, 0), 2, 5)                           # range beyond the reads
    got = fe.run(rec(1, 2, 500, 700, 0), 1, 1)                     # a hang of the whole read
    assert got.shape[0] == 1 and fe.counters() == {"passed": 1, "failed": 0}
    fe.close()


def test_write_red_round_trip(built, tmp_path):
    rs, inp, red, _, _, bgn, end, args = FR.golden("d")
    P, _ = FE.parse_findErrors_args(["-G", "g", "-O", "o", *args])
    fe = FE.FindErrors(P)
    fe.load_reads(rs)
    fe.run(inp, bgn, end)
    p = str(tmp_path / "1.red")
    fe.write_red(p)
    fe.close()
    assert open(p, "rb").read() == red.tobytes()
    assert np.array_equal(FE.read_red(p), red)


def test_chain_from_the_overlapper(built):
    """OverlapInCore.run -> store_view -> FindErrors.run, no file between them."""
    from canu_amd.overlap_in_core import OicParameters, OverlapInCore
    from canu_amd.synth import synth_reads
    rs = synth_reads(n_reads=60, read_len=1500, genome_len=12_000, error_rate=0.01, seed=5)
    P = OicParameters(Kmer_Len=22, maxErate=float(np.float32(0.06)), Min_Olap_Len=100).finalize()
    oic = OverlapInCore(P, device=0)
    ovl = oic.run(rs)
    oic.close()
    store = FE.store_view(ovl)
    assert store.shape[0] == 2 * ovl.shape[0] > 100
    bgn, end = 5, 50
    sel = store[(store["a"] >= bgn) & (store["a"] <= end)]
    o = FR.defaults()
    o["erate"] = 0.045
    fe = FE.FindErrors(_params(o))
    fe.load_reads(rs)
    got = fe.run(sel, bgn, end)
    c = fe.counters()
    fe.close()
    want, p, f = FR.find_errors(sel, FR.reads_dict(rs), bgn, end, o)
    _same(got, want)
    assert c == {"passed": p, "failed": f} and p > 50
    assert ((got["word"] >> 2) & 15 != 0).any()


def test_executable_equals_reference(built, tmp_path):
    """canu's line on a gkpStore and an overlap store the reference wrote: fixture (a)'s bytes
    and the reference's two stderr lines."""
    import subprocess
    import oracle
    from canu_amd.overlap_in_core import write_ovb
    if not (oracle.reference_available() and oracle.store_available()):
        pytest.skip("oracle/_ref/oic_ref and ovs_ref are not built")
    rs, inp, red, passed, failed, bgn, end, args = FR.golden("a")
    both = FE.store_view(inp)                      # every pair once, as an overlapper reports it
    canon = np.unique(both[both["a"] < both["b"]])
    gkp = oracle.build_gkpstore(rs, str(tmp_path))
    ovb = str(tmp_path / "in.ovb")
    write_ovb(canon, ovb, counts=False)
    store = str(tmp_path / "asm.ovlStore")
    oracle.build_store(gkp, store, [ovb])
    out = str(tmp_path / "0001.red.WORKING")
    exe = os.path.join(os.path.dirname(os.path.abspath(FE.__file__)), "bin", "findErrors")
    cp = subprocess.run([exe, "-G", gkp, "-O", store, "-R", str(bgn), str(end), *args, "-l", "500",
                         "-o", out, "-t", "4"], capture_output=True, text=True, timeout=120)
    assert cp.returncode == 0, cp.stderr[-2000:]
    assert open(out, "rb").read() == red.tobytes()
    assert FE.report({"passed": passed, "failed": failed}) in cp.stderr
    # a range whose reads have no overlaps: the IDENT records alone
    empty = str(tmp_path / "none.ovlStore")
    write_ovb(canon[:1], ovb, counts=False)
    oracle.build_store(gkp, empty, [ovb])
    lone = [i for i in range(bgn, end + 1) if i not in (int(canon[0]["a"]), int(canon[0]["b"]))][0]
    cp = subprocess.run([exe, "-G", gkp, "-O", empty, "-R", str(lone), str(lone), "-o", out],
                        capture_output=True, text=True, timeout=120)
    assert cp.returncode == 0, cp.stderr[-2000:]
    got = FE.read_red(out)
    assert got.shape[0] == 1 and int(got[0]["readID"]) == lone and int(got[0]["word"]) == 3
    cp = subprocess.run([exe, "-G", gkp, "-O", str(tmp_path / "absent"), "-R", "1", "2", "-o", out],
                        capture_output=True, text=True, timeout=120)
    assert cp.returncode == 1 and "not an overlap store" in cp.stderr


def _crowd(n, seed):
    """n overlaps among eight reads of about 48 bases of one 64-base stretch, in both
    orientations: every ordered pair of reads, over and over."""
    rng = np.random.default_rng(seed)
    g = _rand(rng, 64)
    reads, where = [], []
    for _ in range(8):
        L = int(rng.integers(44, 53))
        s = int(rng.integers(0, len(g) - L + 1))
        fl = int(rng.integers(0, 2)) if where else 0
        r = _mutate(rng, g[s:s + L], 0.02)
        reads.append(_rc(r) if fl else r)
        where.append((s, s + L, fl))
    assert {fl for _, _, fl in where} == {0, 1}
    pairs = []
    for a in range(8):
        for b in range(8):
            if a == b:
                continue
            (sa, ea, fa), (sb, eb, fb) = where[a], where[b]
            ah = (sb - sa) if fa == 0 else (ea - eb)
            bh = (eb - ea) if fa == 0 else (sa - sb)
            ah = min(max(ah, -(len(reads[b]) - 1)), len(reads[a]) - 1)
            pairs.append(FR.make_record(a + 1, b + 1, ah, bh, fa != fb))
    return reads, [pairs[k % len(pairs)] for k in range(n)]


def test_more_overlaps_than_waves(built):
    """More overlaps than the grid has waves (eight per SIMD): the grid bound decides the number
    of waves and every wave takes several overlaps off the work counter."""
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    reads, recs = _crowd(n_cu * 32 + 7, 57)
    gs, st = _check(reads, recs, 1, len(reads), FR.defaults())
    assert gs["n_passed"] + gs["n_failed"] == len(recs) == n_cu * 32 + 7
    assert gs["regrows"] == 0 and gs["rows"] == st["rows"]
    assert gs["n_passed"] > len(recs) // 2
