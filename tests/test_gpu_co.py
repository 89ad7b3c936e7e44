"""correctOverlaps on the GPU (libcanu_co.so): the reference's .oea bytes and counters on the
fixtures, and the shapes, boundaries, hang and trim cases and error paths against the Python
restatement (tests/co_restate.py, itself pinned to the reference by tests/test_co_cpu.py)."""
import os

import numpy as np
import pytest

import co_restate as CR
import fe_restate as FR
from canu_amd import correct_overlaps as CO
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


def _red(n, cor=None):
    """A .red file for reads 1..n: an IDENT record each, then cor[read] = [(pos, type), ...]."""
    out = []
    for r in range(1, n + 1):
        out.append((3, r))
        for pos, t in (cor or {}).get(r, []):
            out.append((3 | (t << 2) | (pos << 6), r))
    return np.array(out, dtype=CO.RED_DTYPE)


def _records(recs):
    """Distinct nonzero evalues, so that a kept one shows."""
    return np.array([CR.with_evalue(tuple(r), 1 + k % 4000) for k, r in enumerate(recs)],
                    dtype=RECORD_DTYPE)


def _gpu(reads, recs, red, bgn, end, erate, env=None):
    """-> (evalues, counters, stats) of the library."""
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        co = CO.CorrectOverlaps(CO.CoParameters(erate))
        co.load_reads(_read_set(reads))
        co.set_corrections(red)
        out = co.run(recs, bgn, end)
        c, s = co.counters(), co.stats()
        co.close()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    return out, c, s


def _want(reads, recs, red, bgn, end, erate):
    st, br = {}, {}
    ev, c = CR.correct_overlaps(recs, {i + 1: r for i, r in enumerate(reads)}, red, bgn, end,
                                erate, br, st)
    return ev, c, st, br


def _check(reads, recs, red, bgn, end, erate, env=None):
    recs = _records(recs)
    want, wc, st, br = _want(reads, recs, red, bgn, end, erate)
    got, gc, gs = _gpu(reads, recs, red, bgn, end, erate, env)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad[:10], got[bad[:10]], want[bad[:10]])
    assert gc == wc
    assert gs["bases"] == st.get("bases", 0)
    return gs, st, br, got


@pytest.mark.parametrize("name", CR.FIXTURES)
def test_fixture_equals_reference(built, name):
    g = CR.golden(name)
    co = CO.CorrectOverlaps(CO.CoParameters(g["erate"]))
    co.load_reads(g["rs"])
    co.set_corrections(g["red"])
    got = co.run(g["records"], g["bgn"], g["end"])
    assert CO.oea_bytes(g["bgn"], g["end"], got) == g["oea"]
    assert co.counters() == g["counters"]
    assert CO.report(co.counters()) == CO.report(g["counters"])
    co.close()


@pytest.mark.parametrize("L", [1, 31, 32, 33, 63, 64, 65, 2049])
def test_overlap_lengths(built, L):
    """A's last L bases over B's first L, B forward and flipped, with and without errors; a
    deletion and an insertion ahead of the hang move it."""
    rng = np.random.default_rng(100 + L)
    reads, recs, cor = [], [], {}
    for err in (0.0, 0.05):
        for fl in (0, 1):
            x = _rand(rng, L)
            a = _rand(rng, 300) + x
            y = _mutate(rng, x, err) if L > 8 else x
            b = (y or x[:1]) + _rand(rng, 300)
            reads += [a, _rc(b) if fl else b]
            recs.append(FR.make_record(len(reads) - 1, len(reads), 300, 300, fl))
            if err:
                cor[len(reads) - 1] = [(100, FR.DELETE), (200, FR.A_INSERT), (250, FR.A_INSERT)]
    _check(reads, recs, _red(len(reads), cor), 1, len(reads), 0.144)


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
    """Widest rows of CO_WINDOW_DIAGS - 1, CO_WINDOW_DIAGS and + 1 diagonals; the last leave the
    register window for the path that reads the row before from the row log."""
    a, b = _periodic(n, cut)
    recs = [FR.make_record(1, 2, 0, 0, 0), FR.make_record(2, 1, 0, 0, 0)]
    gs, st, _, _ = _check([a, b], recs[:1], _red(2), 1, 2, 0.144)
    assert st["max_width"] == width                      # the restatement's own band
    assert gs["n_generic"] == (1 if width > CO.WINDOW_DIAGS else 0)
    assert gs["rows"] == st["rows"] and gs["regrows"] == 0
    _check([a, b], recs, _red(2), 1, 2, 0.144)


@pytest.mark.parametrize("side", ["a", "b"])
@pytest.mark.parametrize("span", [CO.LDS_BASES - 1, CO.LDS_BASES, CO.LDS_BASES + 1])
def test_lds_strand_capacity(built, span, side):
    """The longer reachable span of CO_LDS_BASES - 1, CO_LDS_BASES and + 1 bases: up to the
    capacity both spans are staged in LDS, past it on either side the alignment reads global
    memory.  The other read ends 100 bases short, less than the errors allowed, so the long span
    is reachable to its end.  The long read loses a base ahead of the hang and gains one inside
    the span: the span is counted on the corrected read."""
    rng = np.random.default_rng(span)
    x = _rand(rng, span - 1)                              # + 1 inserted base: the span
    y = _mutate(rng, x[:span - 100], 0.03)
    reads, recs, cor = [], [], {}
    for fl in (0, 1):
        if side == "a":                      # a_part is the long span, B ends inside it
            a, b, ah, bh = _rand(rng, 408) + x, y, 408, -100
            long_read, at = len(reads) + 1, 408 + 3000
        else:                                # b_part is the long span, A ends inside it
            a, b, ah, bh = y, _rand(rng, 422) + x, -422, 100
            long_read, at = len(reads) + 2, ((span - 1) - 3000) if fl else 422 + 3000
        reads += [a, _rc(b) if fl else b]
        recs.append(FR.make_record(len(reads) - 1, len(reads), ah, bh, fl))
        # on a flipped B the hang counts from the other end: the deletion goes there
        dele = (len(reads[long_read - 1]) - 50) if (side == "b" and fl) else 50
        cor[long_read] = sorted([(dele, FR.DELETE), (at, FR.C_INSERT)])
    short = [_rand(rng, 300) + x[:900], x[:900] + _rand(rng, 200)]     # one that is staged anyway
    reads += short
    recs.append(FR.make_record(len(reads) - 1, len(reads), 300, 200, 0))
    gs, st, _, _ = _check(reads, recs, _red(len(reads), cor), 1, len(reads), 0.06)
    assert gs["n_staged"] == (3 if span <= CO.LDS_BASES else 1)
    assert gs["rows"] == st["rows"] > 100 and gs["regrows"] == 0


@pytest.mark.parametrize("delta,regrows", [(-1, 1), (0, 0), (1, 0)])
def test_row_log_boundary_and_regrow(built, delta, regrows):
    """A first row log one entry short of what the alignment writes is an overflow: the overlap
    runs again with the worst-case log and gives the same bytes."""
    rng = np.random.default_rng(7)
    x = _rand(rng, 1500)
    reads = [x, _mutate(rng, x, 0.06), _rand(rng, 400) + x[:900], _mutate(rng, x[300:], 0.03)]
    recs = [FR.make_record(1, 2, 0, len(reads[1]) - 1500, 0)]
    red = _red(4, {1: [(700, FR.G_SUBST)]})
    _, _, st, _ = _want(reads, _records(recs), red, 1, 1, 0.144)
    gs, _, _, first = _check(reads, recs, red, 1, 1, 0.144, {"CANU_CO_LOG_CAP": str(st["log_used"] + delta)})
    assert gs["regrows"] == regrows
    # among others that fit: only the overflowing ones run again, and nothing is counted twice
    recs += [FR.make_record(1, 3, -400, -600, 0), FR.make_record(1, 4, 300, 0, 0)]
    gs, _, _, got = _check(reads, recs, red, 1, 1, 0.144, {"CANU_CO_LOG_CAP": str(st["log_used"] + delta)})
    assert gs["regrows"] == regrows and got[0] == first[0]
    gs, _, _, _ = _check(reads, recs, red, 1, 1, 0.144, {"CANU_CO_LOG_PER_ERROR": "1"})
    assert gs["regrows"] == 1


def test_hang_against_adjust_positions(built):
    """The stored hang one short of, on and one past an adjust position, for the A list, the
    forward B list and the reverse B list; the read has a deletion, an insertion and a
    substitution followed by an insertion at one base."""
    rng = np.random.default_rng(11)
    raw = _rand(rng, 900)
    cor = {1: [(200, FR.DELETE), (400, FR.T_INSERT), (600, FR.C_SUBST), (600, FR.G_INSERT)]}
    red0 = _red(1, cor)
    seq, fadj, _ = CR.correct_read(1, FR.filter_read(raw), red0, 0)
    radj = CR.make_rev_adjust(fadj, seq.shape[0])
    assert len(fadj) == len(radj) == 3
    T = _ACGT[seq].tobytes()                              # the corrected read
    reads, recs = [raw], []
    for which, lst in (("a", fadj), ("bf", fadj), ("br", radj)):
        for adjpos, _ in lst:
            for d in (-1, 0, 1):
                h = adjpos + d
                if which == "a":
                    reads.append(T[h:] + _rand(rng, 120))
                    recs.append(FR.make_record(1, len(reads), h, 120, 0))
                elif which == "bf":
                    reads.append(T[h:] + _rand(rng, 120))
                    recs.append(FR.make_record(len(reads), 1, -h, -120, 0))
                else:
                    reads.append(_rc(T)[h:] + _rand(rng, 120))
                    recs.append(FR.make_record(len(reads), 1, -h, -120, 1))
    red = _red(len(reads), cor)
    _, _, br, got = _check(reads, recs, red, 1, len(reads), 0.06)
    for w in ("a", "b_fwd", "b_rev"):
        for t in ("m1", "0", "p1"):
            assert br.get(f"at_{w}_{t}", 0) >= 3, (w, t, br)
    assert br["insert_after_subst"] and br["insert_copy"] and br["rev_adjust"]
    assert (got == 0).sum() >= 9                          # where the adjusted hang is the true one


def _trim_job(seed):
    """Reads with leading bases their partner lacks, on A and on B, B forward and flipped, with
    the stored hang below the gap's length (i == stop), above it with another gap further on
    (i < stop), and above it with no other gap (deltaLen < |a_hang|)."""
    rng = np.random.default_rng(seed)
    reads, recs = [], []
    for fl in (0, 1):
        o = _rc if fl else (lambda s: s)
        for lead, later_gap in ((2, False), (10, True), (10, False)):
            core = bytearray(_rand(rng, 420))
            if core[0] == ord("T"):
                core[0] = ord("A")
            long_side = bytearray(core) + _rand(rng, 60)
            if later_gap:
                del long_side[200]
            pre = _rand(rng, lead)
            reads += [pre + b"TTT" + bytes(core), o(bytes(long_side))]       # the extra bases on A
            recs.append(FR.make_record(len(reads) - 1, len(reads), lead, 60, fl))
            reads += [bytes(long_side), o(pre + b"TTT" + bytes(core))]       # the extra bases on B
            recs.append(FR.make_record(len(reads) - 1, len(reads), -lead, -60, fl))
    return reads, recs


def test_leading_gap_trims(built):
    reads, recs = _trim_job(5)
    _, wc, br, got = _check(reads, recs, _red(len(reads)), 1, len(reads), 0.06)
    for k in ("trim_a_stop", "trim_a_short", "trim_a_all", "trim_b_stop", "trim_b_short", "trim_b_all"):
        assert br.get(k, 0) >= 2, (k, br)
    assert (got <= 30).all()                              # the gap came off the error count


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
    """With the .red file findErrors gives for the same reads and overlaps."""
    reads, recs = _sample(31)
    n = len(reads)
    all_recs = np.array(recs, dtype=RECORD_DTYPE)
    fe = FE.FindErrors(FE.FeParameters(error_rate=0.045))
    fe.load_reads(_read_set(reads))
    red = fe.run(all_recs, 1, n)
    fe.close()
    assert ((red["word"] >> 2) & 15 != 0).sum() > 20
    sel = _records([r for r in recs if 3 <= r[0] <= n - 2])
    want, wc, _, _ = _want(reads, sel, red, 3, n - 2, 0.045)
    co = CO.CorrectOverlaps(CO.CoParameters(0.045))
    co.load_reads(_read_set(reads))
    co.set_corrections(red)
    first, c1 = co.run(sel, 3, n - 2), co.counters()
    assert np.array_equal(first, want) and c1 == wc and wc["total"] - wc["failed_either"] > 50
    again, c2 = co.run(sel, 3, n - 2), co.counters()
    perm = np.random.default_rng(1).permutation(sel.shape[0])
    other, c3 = co.run(sel[perm], 3, n - 2), co.counters()
    co.set_corrections(red)                               # a second set of the same corrections
    fresh, c4 = co.run(sel, 3, n - 2), co.counters()
    co.close()
    assert np.array_equal(again, first) and np.array_equal(other, first[perm])
    assert np.array_equal(fresh, first) and c1 == c2 == c3 == c4


def test_range_and_error_behaviour(built, tmp_path):
    rng = np.random.default_rng(3)
    reads = [_rand(rng, 500), _rand(rng, 700), _rand(rng, 300)]
    rec = lambda *a: np.array([CR.with_evalue(FR.make_record(*a), 77)], dtype=RECORD_DTYPE)
    co = CO.CorrectOverlaps()
    co.load_reads(_read_set(reads))
    with pytest.raises(CO.CoError) as e:                  # no corrections yet
        co.run(rec(1, 2, 0, 0, 0), 1, 3)
    assert e.value.code == -7
    co.set_corrections(_red(3))
    got = co.run(np.zeros(0, dtype=RECORD_DTYPE), 1, 3)   # the empty range
    assert got.shape == (0,) and got.dtype == np.uint16
    c = co.counters()
    assert all(c[k] == 0 for k in CO.COUNTERS) and c["corrected_bases"] == 1503
    p = str(tmp_path / "empty.oea")
    co.write_oea(p)
    assert open(p, "rb").read() == CO.oea_bytes(1, 3, got) and os.path.getsize(p) == 16
    for bad in (rec(3, 1, 0, 0, 0), rec(1, 4, 0, 0, 0)):  # a_iid outside, b not loaded
        with pytest.raises(CO.CoError) as e:
            co.run(bad, 1, 2)
        assert e.value.code == -4
    for bad in (rec(1, 2, 501, 0, 0), rec(1, 3, -301, 0, 1), rec(1, 3, -301, 0, 0)):
        with pytest.raises(CO.CoError) as e:              # the adjusted hang beyond its read
            co.run(bad, 1, 3)
        assert e.value.code == -4
    with pytest.raises(CO.CoError):
        co.run(rec(1, 2, 0, 0, 0), 2, 5)                  # range beyond the reads
    got = co.run(rec(1, 2, 500, 700, 0), 1, 1)            # a hang of the whole read: length 0
    assert got.tolist() == [77] and co.counters()["failed_length"] == 1
    # a deletion ahead of the hang brings a hang of the whole read + 1 back inside
    co.set_corrections(_red(3, {1: [(10, FR.DELETE)]}))
    assert co.run(rec(1, 2, 500, 700, 0), 1, 1).tolist() == [77]
    with pytest.raises(CO.CoError) as e:
        co.run(rec(1, 2, 501, 700, 0), 1, 1)
    assert e.value.code == -4
    # corrections: not ascending; no IDENT record for a needed read; the position assertion
    red = _red(3)
    with pytest.raises(CO.CoError) as e:
        co.set_corrections(red[::-1])
    assert e.value.code == -4
    with pytest.raises(CO.CoError) as e:                  # ... and that dropped the corrections
        co.run(rec(1, 2, 0, 0, 0), 1, 1)
    assert e.value.code == -7
    co.set_corrections(red[red["readID"] != 2])
    with pytest.raises(CO.CoError) as e:
        co.run(rec(1, 2, 0, 0, 0), 1, 1)                  # B needs it
    assert e.value.code == -4 and "IDENT" in str(e.value)
    with pytest.raises(CO.CoError) as e:
        co.run(rec(1, 3, 0, 0, 0), 1, 2)                  # the range needs it
    assert e.value.code == -4
    assert co.run(rec(1, 3, 0, 0, 0), 1, 1).shape == (1,)  # nobody needs it
    for cor in ([(10, FR.C_SUBST), (5, FR.C_SUBST)], [(10, FR.C_SUBST), (10, FR.G_SUBST), (10, FR.A_INSERT)],
                [(10, 11)]):
        bad_red = _red(3, {2: cor})
        with pytest.raises(CR.BadInput):
            CR.correct_read(2, FR.filter_read(reads[1]), bad_red, 0)
        co.set_corrections(bad_red)
        with pytest.raises(CO.CoError) as e:
            co.run(rec(1, 2, 0, 0, 0), 1, 1)
        assert e.value.code == -4
        assert co.run(rec(1, 3, 0, 0, 0), 1, 1).shape == (1,)
    # a correction beyond the read's end is never reached (correctRead's loop ends first)
    late = _red(3, {2: [(699, FR.C_SUBST), (699, FR.A_INSERT), (5000, FR.DELETE)]})
    co.close()
    _check(reads, [FR.make_record(1, 2, 0, 200, 0), FR.make_record(2, 1, 0, -200, 0)], late, 1, 3, 0.06)


def test_reads_from_device_buffers_and_oea_file(built, tmp_path):
    """The buffers fe_load_reads_device takes (lower-case and N bytes among them), a second
    load, and the file the library writes."""
    import torch
    g = CR.golden("d")
    rs = g["rs"]
    low = np.array(rs.bases)
    low[::3] |= 0x20                                      # a third of the bases in lower case
    d_bases = torch.from_numpy(low).cuda()
    d_offs = torch.from_numpy(np.array(rs.offsets).astype(np.int64)).cuda()
    torch.cuda.synchronize()
    co = CO.CorrectOverlaps(CO.CoParameters(g["erate"]))
    co.load_reads(CR.golden("e")["rs"])                   # replaced by the next load
    co.load_reads_device(rs.first_iid, d_bases.data_ptr(), d_offs.data_ptr(), rs.lengths)
    with pytest.raises(CO.CoError) as e:                  # a load drops the corrections
        co.run(g["records"], g["bgn"], g["end"])
    assert e.value.code == -7
    co.set_corrections(g["red"])
    got = co.run(g["records"], g["bgn"], g["end"])
    p = str(tmp_path / "d.oea")
    co.write_oea(p)
    assert co.counters() == g["counters"]
    co.close()
    assert open(p, "rb").read() == g["oea"]
    bgn, end, ev = CO.read_oea(p)
    assert (bgn, end) == (g["bgn"], g["end"]) and np.array_equal(ev, got)


def test_chain_from_the_overlapper(built):
    """OverlapInCore.run -> store_view -> FindErrors.run -> CorrectOverlaps.run -> apply_evalues,
    no file between them."""
    from canu_amd.overlap_in_core import OicParameters, OverlapInCore
    from canu_amd.synth import synth_reads
    rs = synth_reads(n_reads=60, read_len=1500, genome_len=12_000, error_rate=0.01, seed=5)
    P = OicParameters(Kmer_Len=22, maxErate=float(np.float32(0.06)), Min_Olap_Len=100).finalize()
    oic = OverlapInCore(P, device=0)
    ovl = oic.run(rs)
    oic.close()
    store = FE.store_view(ovl)
    assert store.shape[0] == 2 * ovl.shape[0] > 100
    fe = FE.FindErrors(FE.FeParameters(error_rate=0.045))
    fe.load_reads(rs)
    red = fe.run(store, 1, rs.nreads)
    fe.close()
    bgn, end = 5, 50
    sel = store[(store["a"] >= bgn) & (store["a"] <= end)]
    co = CO.CorrectOverlaps(CO.CoParameters(0.045))
    co.load_reads(rs)
    co.set_corrections(red)
    got = co.run(sel, bgn, end)
    c = co.counters()
    co.close()
    want, wc = CR.correct_overlaps(sel, FR.reads_dict(rs), red, bgn, end, 0.045)
    assert np.array_equal(got, want) and c == wc
    assert c["total"] == sel.shape[0] and c["total"] - c["failed_either"] > 50
    assert c["substitutions"] + c["deletions"] + c["insertions"] > 0
    came = CO.evalues_of(sel)
    assert (got < came).sum() > (got > came).sum()        # corrected reads agree better
    out = CO.apply_evalues(sel, got)
    assert np.array_equal(CO.evalues_of(out), got) and np.array_equal(out["b"], sel["b"])


def test_executable_equals_reference(built, tmp_path):
    """canu's line on a gkpStore and an overlap store the reference wrote: fixture (a)'s bytes
    and the reference's stderr lines; the store with an evalues file; the empty range."""
    import subprocess
    import oracle
    from canu_amd.overlap_in_core import write_ovb
    if not (oracle.reference_available() and oracle.store_available()):
        pytest.skip("oracle/_ref/oic_ref and ovs_ref are not built")
    g = CR.golden("a")
    rs, inp, bgn, end = g["rs"], g["records"], g["bgn"], g["end"]
    both = FE.store_view(inp)                      # every pair once, as an overlapper reports it
    canon = np.unique(both[both["a"] < both["b"]])
    gkp = oracle.build_gkpstore(rs, str(tmp_path))
    ovb = str(tmp_path / "in.ovb")
    write_ovb(canon, ovb, counts=False)
    store = str(tmp_path / "asm.ovlStore")
    oracle.build_store(gkp, store, [ovb])
    red = str(tmp_path / "red.red")
    open(red, "wb").write(g["red"].tobytes())
    out = str(tmp_path / "00001.oea.WORKING")
    exe = os.path.join(os.path.dirname(os.path.abspath(CO.__file__)), "bin", "correctOverlaps")
    line = [exe, "-G", gkp, "-O", store, "-R", str(bgn), str(end), "-e", repr(g["erate"]), "-l",
            "500", "-c", red, "-o", out]
    cp = subprocess.run(line, capture_output=True, text=True, timeout=120)
    assert cp.returncode == 0, cp.stderr[-2000:]
    assert open(out, "rb").read() == g["oea"]
    assert CO.report(g["counters"]) in cp.stderr
    # a range whose reads have no overlaps: a header with n = 0
    empty = str(tmp_path / "none.ovlStore")
    write_ovb(canon[:1], ovb, counts=False)
    oracle.build_store(gkp, empty, [ovb])
    lone = [i for i in range(bgn, end + 1) if i not in (int(canon[0]["a"]), int(canon[0]["b"]))][0]
    cp = subprocess.run([exe, "-G", gkp, "-O", empty, "-R", str(lone), str(lone), "-c", red, "-o", out],
                        capture_output=True, text=True, timeout=120)
    assert cp.returncode == 0, cp.stderr[-2000:]
    assert open(out, "rb").read() == CO.oea_bytes(lone, lone, np.zeros(0, dtype=np.uint16))
    # a store whose error rates were adjusted already
    open(os.path.join(store, "evalues"), "wb").write(b"\0" * 8)
    os.remove(out)
    cp = subprocess.run(line, capture_output=True, text=True, timeout=120)
    assert cp.returncode == 1 and "evalues" in cp.stderr and not os.path.exists(out)
    cp = subprocess.run([exe, "-G", gkp, "-O", empty, "-R", "1", "2", "-c", str(tmp_path / "absent"),
                         "-o", out], capture_output=True, text=True, timeout=120)
    assert cp.returncode == 1 and "can't open" in cp.stderr


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
    of waves and every wave takes several overlaps off the work counter.  Two reads carry a
    correction, so hangs are adjusted on the way."""
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    reads, recs = _crowd(n_cu * 32 + 7, 57)
    red = _red(len(reads), {2: [(20, FR.DELETE)], 5: [(10, FR.A_INSERT), (30, FR.C_SUBST)]})
    gs, st, _, got = _check(reads, recs, red, 1, len(reads), 0.06)
    assert gs["total"] == len(recs) == n_cu * 32 + 7
    assert gs["regrows"] == 0 and gs["rows"] == st["rows"]
    assert gs["total"] - gs["failed_either"] > len(recs) // 2
