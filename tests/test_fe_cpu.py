"""findErrors' host side, with no GPU: the Python restatement against the reference's fixtures,
the store view against the reference's store, the argument line and the .red helpers."""
import os

import numpy as np
import pytest

import fe_restate as FR
import fe_votes as FV
import oracle
from canu_amd import find_errors as FE
from canu_amd.overlap_in_core import RECORD_DTYPE, write_ovb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", FR.FIXTURES)
def test_restatement_equals_reference(built, name):
    """Pins tests/fe_restate.py to the reference findErrors: every byte, both counters."""
    rs, inp, red, passed, failed, bgn, end, args = FR.golden(name)
    got, p, f = FR.find_errors(inp, FR.reads_dict(rs), bgn, end, FR.parse_args(args))
    assert got.tobytes() == red.tobytes(), FE.dump_red(got[:30]) + "\n" + FE.dump_red(red[:30])
    assert (p, f) == (passed, failed)


def test_fixtures_cover_the_cases(built):
    """What the fixtures are for shows in the reference's own output."""
    types = set()
    for n in FR.FIXTURES:
        rs, inp, red, passed, failed, bgn, end, args = FR.golden(n)
        assert passed > 0 and failed > 0, n
        t = (red["word"] >> 2) & 15
        types |= set(int(v) for v in t)
        ids, cnt = np.unique(red["readID"], return_counts=True)
        assert ids.tolist() == list(range(bgn, end + 1)) and (cnt == 1).any(), n
        assert (inp["a"] >= bgn).all() and (inp["a"] <= end).all()
        assert ((inp["w0"] >> np.uint64(54)) & np.uint64(1)).any(), n
    assert types == set(range(10))                    # IDENT and the nine votes
    rs, inp, red, _, _, bgn, end, _ = FR.golden("d")
    keep = red["word"][(red["word"] >> 2) & 15 == 0] & 3
    assert set(int(v) & 1 for v in keep) == {0, 1} and set(int(v) >> 1 for v in keep) == {0, 1}
    assert b"N" in rs.bases.tobytes()
    assert (inp["b"] > end).sum() > 255               # B reads outside the range, > 255 deep
    st = {}
    FR.find_errors(inp, FR.reads_dict(rs), bgn, end, FR.defaults(), st)
    assert st["rescued"] >= 2                         # Process_Olap :149-152, both strands
    c = FR.golden("c")
    o = FR.parse_args(c[7])
    assert not o["use_haplo_ct"] and o["degree_threshold"] == 4
    o["use_haplo_ct"] = True                          # the haplotype count matters there
    got, _, _ = FR.find_errors(c[1], FR.reads_dict(c[0]), c[5], c[6], o)
    assert got.shape[0] < c[2].shape[0]


def _walked(name):
    """A fixture through the restatement and the instrumented ladders -> (counts, stats, P)."""
    rs, inp, red, passed, failed, bgn, end, args = FR.golden(name)
    P = FR.parse_args(args)
    st = {}
    reads = FR.reads_dict(rs)
    got, p, f = FR.find_errors(inp, reads, bgn, end, P, st)
    again, n = FV.walk(st["tallies"], st["degrees"], reads, bgn, end, P)
    assert got.tobytes() == again.tobytes() == red.tobytes(), name
    return n, st, P


def test_fixtures_reach_every_branch(built):
    """Every branch of the two Output_Corrections ladders and every constructed case is in some
    fixture, so the reference's own bytes back it: fe_votes.REQUIRED, counted by the ladders
    walked once more with a counter on every branch, whose records equal the reference's."""
    total = FV.collections.Counter()
    seen = {}
    for name in FR.FIXTURES:
        n, st, P = _walked(name)
        total.update(n)
        seen[name] = (n, st, P)
        if name in FV.LINES:                  # nothing voted outside a read in the constructed ones
            assert st.get("outside", 0) == 0 and FR.golden(name)[7] == FV.LINES[name]
    assert not [k for k in FV.REQUIRED if total[k] == 0]
    # with -x 0 nothing votes for A's own letter (fe_votes' docstring): the one row of the
    # table that no input reaches
    assert total["!is_change with -x 0"] == 0
    assert all(seen[k][2]["end_exclude_len"] == 0 for k in "bgi")
    # what the single fixtures are for
    for k in "eh":
        assert seen[k][0]["insert record"] == 0 and seen[k][0]["haplo_ct >= 2, refused"] > 0
    assert seen["f"][0]["two records at the last base of a block"] == 1
    assert seen["g"][0]["ins_haplo_ct >= 2, refused"] > 0
    assert seen["i"][0]["insert plane at MAX_VOTE"] == 1
    # kmer_len < 2 * end_exclude_len: runs of K, 2X - 1, 2X and 2X + 1 between two changes, at
    # the alignment's start and at its end, from overlaps with a_hang > 0 and without
    n, st, P = seen["h"]
    K, X = P["kmer_len"], P["end_exclude_len"]
    assert K < 2 * X and st["fs_skipped"] > 0
    for r in (K, 2 * X - 1, 2 * X, 2 * X + 1):
        for hang in (False, True):
            assert (r, False, False, hang) in st["runs"], (r, hang)
            assert (r, False, True, hang) in st["runs"], (r, hang)
        assert (r, True, False, True) in st["runs"], r
    assert (2 * X - 1, True, False, False) in st["runs"]


def _fresh_reference(lab):
    """The restatement against a fresh run of the reference findErrors on a lab job."""
    from canu_amd.synth import ReadSet
    if not oracle.fe_reference_available():               # asked after `built`, which makes it
        pytest.skip("oracle/_ref/fe_ref, oic_ref and ovs_ref are not built")
    reads, recs, bgn, end, want, p, f, st = FV.restate(lab)
    lens = np.array([len(r) for r in reads], dtype=np.uint32)
    offs = np.zeros(len(reads), dtype=np.uint64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    rs = ReadSet(bases=np.frombuffer(b"".join(reads), dtype=np.uint8).copy(), offsets=offs,
                 lengths=lens, first_iid=1)
    raw, rp, rf, sel = oracle.run_find_errors(rs, np.array(recs, dtype=RECORD_DTYPE), bgn, end,
                                              lab.args)
    assert sel.shape[0] == len(recs)
    ref = np.frombuffer(raw, dtype=FR.RED_DTYPE)
    assert want.tobytes() == ref.tobytes(), FE.dump_red(want[:30]) + "\n" + FE.dump_red(ref[:30])
    assert (p, f) == (rp, rf)
    return want


@pytest.mark.parametrize("line", sorted(FV.LINES))
def test_restatement_equals_fresh_reference(built, line):
    """Random small tallies at 20 sites, three seeds, under each option line."""
    records = 0
    for seed in (11, 12, 13):
        lab = FV.Lab(seed * 100 + ord(line), FV.LINES[line])
        FV.random_sites(lab, 20)
        lab.false_pair(0)
        red = _fresh_reference(lab)
        records += int(((red["word"] >> 2) & 15 != 0).sum())
    assert records > 0


@pytest.mark.parametrize("plane,line", [
    ("subst", "f"), ("subst_confirmed_1", "e"), ("confirmed", "e"), ("insert", "i"),
    ("insert_no_insert_1", "i"), ("no_insert", "g")])
def test_saturation_equals_fresh_reference(built, plane, line):
    """255, 256 and 300 votes on every plane of the tally: MAX_VOTE holds each of them."""
    lab = FV.Lab(77, FV.LINES[line])
    for n in (255, 256, 300):
        FV.saturation(lab, plane, n)
    _fresh_reference(lab)


def test_aligner_by_hand():
    """Exact prefix, one substitution, the branch-point exit and the forced mismatch."""
    f = FR.filter_read
    ML = FR.match_limit(0.06, 64)
    assert FR.prefix_edit_dist(f(b"ACGTACGT"), f(b"ACGTACGTAA"), 2, 0.06, ML) == (0, 8, 8, True, [])
    a = b"ACGTTGCAAGCT" * 4
    b = bytearray(a)
    b[20] = ord("A") if a[20] != ord("A") else ord("C")
    e, ae, be, to_end, delta = FR.prefix_edit_dist(f(a), f(bytes(b)), 3, 0.06, ML)
    assert (e, ae, be, to_end, delta) == (1, 48, 48, True, [])
    e, ae, be, to_end, delta = FR.prefix_edit_dist(f(a), f(bytes(b[:20] + b[21:])), 3, 0.06, ML)
    assert (e, ae, be, to_end) == (1, 48, 47, True) and delta == [21]
    e, ae, be, to_end, delta = FR.prefix_edit_dist(f(a[:20] + a[21:]), f(a), 3, 0.06, ML)
    assert (e, ae, be, to_end) == (1, 47, 48, True) and delta == [-21]
    assert FR.filter_read(b"acgtNnXACGT").tolist() == [0, 1, 2, 3, 0, 0, 0, 0, 1, 2, 3]
    assert FR.error_bound(1000, 0.045) == 45 and FR.error_bound(1001, 0.045) == 46


def test_parse_canu_line():
    """red.sh's line (OverlapErrorAdjustment.pm:194-202)."""
    line = ("-G ../asm.gkpStore -O ../asm.ovlStore -R 1 4500 -e 0.045 -l 500 "
            "-o ./0001.red.WORKING -t 8").split()
    P, job = FE.parse_findErrors_args(line)
    assert P == FE.FeParameters(error_rate=0.045)
    assert (job["gkp"], job["ovl"], job["out"]) == ("../asm.gkpStore", "../asm.ovlStore",
                                                    "./0001.red.WORKING")
    assert (job["bgn"], job["end"], job["threads"], job["min_overlap"]) == (1, 4500, 8, 500)
    P, job = FE.parse_findErrors_args("-G g -O o -d 4 -k 8 -V 6 -x 0 -p".split())
    assert P == FE.FeParameters(0.06, 4, 8, 6, 0, False)
    assert job["out"] is None and job["end"] == 0xFFFFFFFF
    for bad in ("-O o", "-G g", "-G g -O o -z", "-G g -O o -R 1", "-G g -O o -t 0"):
        with pytest.raises(ValueError):
            FE.parse_findErrors_args(bad.split())
    assert FR.parse_args("-e 0.144 -k 8 -V 6 -x 0 -p -d 4".split()) == {
        "erate": 0.144, "degree_threshold": 4, "kmer_len": 8, "vote_qualify_len": 6,
        "end_exclude_len": 0, "use_haplo_ct": False}


def test_red_helpers(tmp_path):
    _, _, red, passed, failed, _, _, _ = FR.golden("b")
    p = str(tmp_path / "b.red")
    red.tofile(p)
    assert np.array_equal(FE.read_red(p), red) and FE.RED_DTYPE == FR.RED_DTYPE
    txt = FE.dump_red(red).splitlines()
    assert len(txt) == red.shape[0]
    first = red[0]
    assert txt[0] == "%8u %12s %8u %c %c" % (first["readID"], "IDENT", 0,
                                             "ft"[first["word"] & 1], "ft"[(first["word"] >> 1) & 1])
    k = int(np.nonzero((red["word"] >> 2) & 15 == FR.G_INSERT)[0][0])
    assert txt[k].split()[1] == "G_INSERT" and int(txt[k].split()[2]) == red[k]["word"] >> 6
    rep = FE.report({"passed": passed, "failed": failed})
    assert rep.splitlines()[0] == "Passed overlaps = %10d %8.4f%%" % (
        passed, 100.0 * passed / (passed + failed))
    assert FE.report({"passed": 0, "failed": 0}).splitlines()[1] == \
        "Failed overlaps =          0     -nan%"


def test_store_view_by_hand():
    r = np.array([FR.make_record(7, 3, 120, -40, 1), FR.make_record(2, 9, -5, 60, 0),
                  (4, 5, 0, 0)], dtype=RECORD_DTYPE)          # the last has no for-flag: dropped
    s = FE.store_view(r)
    assert [(int(x["a"]), int(x["b"])) for x in s] == [(2, 9), (3, 7), (7, 3), (9, 2)]
    o = {(int(x["a"]), int(x["b"])): FR.unpack_olap(x)[2:] for x in s}
    assert o[(7, 3)] == (120, -40, 1) and o[(2, 9)] == (-5, 60, 0)
    assert o[(9, 2)] == (5, -60, 0)                           # swapIDs, not flipped
    assert o[(3, 7)] == (-40, 120, 1)                         # flipped: the hangs cross


@pytest.mark.skipif(not (oracle.reference_available() and oracle.store_available()),
                    reason="oracle/_ref/oic_ref and ovs_ref are not built")
def test_store_view_equals_the_reference_store(built, tmp_path):
    rs, _, _, _, _, _, _, _ = FR.golden("d")
    rng = np.random.default_rng(4)
    n = rs.nreads
    recs = []
    for _ in range(300):
        a, b = (int(v) for v in rng.integers(1, n + 1, 2))
        if a == b:
            continue
        la, lb = int(rs.lengths[a - 1]), int(rs.lengths[b - 1])
        recs.append(FR.make_record(a, b, int(rng.integers(-lb + 1, la)),
                                   int(rng.integers(-la + 1, lb)), int(rng.integers(0, 2))))
    inp = np.array(recs, dtype=RECORD_DTYPE)
    gkp = oracle.build_gkpstore(rs, str(tmp_path))
    ovb = str(tmp_path / "in.ovb")
    write_ovb(inp, ovb, counts=False)
    store = str(tmp_path / "t.ovlStore")
    assert oracle.build_store(gkp, store, [ovb]) == 2 * inp.shape[0]
    assert np.array_equal(FE.store_view(inp), oracle.dump_store(gkp, store))


def test_library_exports_and_parameter_checks(built):
    lib = FE.load_library()
    assert not [e for e in FE.EXPORTS if not hasattr(lib, e)]
    assert lib.fe_abi_version() == FE.ABI_VERSION
    p = FE._Params()
    lib.fe_params_init(p)
    assert (p.error_rate, p.degree_threshold, p.kmer_len, p.vote_qualify_len, p.end_exclude_len,
            p.use_haplo_ct) == (0.06, 2, 9, 9, 3, 1)
    hdr = open(os.path.join(ROOT, "include", "canu_fe.h")).read()
    assert f"#define FE_WINDOW_DIAGS {FE.WINDOW_DIAGS}\n" in hdr
    assert f"#define FE_LOG_PER_ERROR {FE.LOG_PER_ERROR}\n" in hdr
    assert f"#define FE_LDS_BASES {FE.LDS_BASES}\n" in hdr
    assert f"#define FE_ABI_VERSION {FE.ABI_VERSION}\n" in hdr


# ----------------------------------------------------------------------- the overlap store reader

@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """tests/fe_host_check.cpp under AddressSanitizer and UBSan, a program of its own."""
    import shutil
    import subprocess
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no C++ compiler"
    exe = str(tmp_path_factory.mktemp("fe_host") / "fe_host_check")
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "fe_host_check.cpp")], check=True, timeout=300)
    return exe


def _store_fixture():
    z = np.load(os.path.join(FR.GOLDEN, "fe_store.npz"))
    files = {str(n): z["file_" + str(n)].tobytes() for n in z["names"]}
    rec = np.zeros(z["rec_a"].shape[0], dtype=RECORD_DTYPE)
    for f in RECORD_DTYPE.names:
        rec[f] = z["rec_" + f]
    return files, rec, [tuple(int(v) for v in r) for r in z["ranges"]]


def _write_store(d, files):
    os.makedirs(d, exist_ok=True)
    for n, b in files.items():
        with open(os.path.join(d, n), "wb") as f:
            f.write(b)
    return str(d)


def _read_store(exe, store, bgn, end, tmp_path):
    import subprocess
    out = str(tmp_path / "rec.bin")
    cp = subprocess.run([exe, "read", store, str(bgn), str(end), out], capture_output=True,
                        text=True, timeout=120)
    return cp, (np.fromfile(out, dtype=RECORD_DTYPE) if cp.returncode == 0 else None)


def test_store_reader_reads_the_reference_store(host_check, tmp_path):
    files, rec, ranges = _store_fixture()
    store = _write_store(tmp_path / "s.ovlStore", files)
    assert rec.shape[0] > 100 and ranges[0] == (3, 9)
    for bgn, end in ranges + [(1, 0xFFFFFFFF), (7, 7), (9, 3), (int(rec["a"].max()) + 1, 10 ** 6)]:
        cp, got = _read_store(host_check, store, bgn, end, tmp_path)
        assert cp.returncode == 0, cp.stderr
        want = rec[(rec["a"] >= bgn) & (rec["a"] <= end)]
        assert np.array_equal(got, want), (bgn, end)
    assert not (rec["a"] == 7).any() and (rec["a"] == 8).any()      # a read with no overlaps
    # the same overlaps in two data files, a read's overlaps running on into the second
    k = int(np.nonzero(rec["a"] == 8)[0][0]) + 1
    two = dict(files)
    two["0001"], two["0002"] = files["0001"][:20 * k], files["0001"][20 * k:]
    info = np.frombuffer(files["info"], dtype="<u8").copy()
    info[6] = 2
    two["info"] = info.tobytes()
    idx = np.frombuffer(files["index"], dtype=np.dtype([("a", "<u4"), ("f", "<u4"), ("o", "<u4"),
                                                        ("n", "<u4"), ("id", "<u8")])).copy()
    later = idx["o"] >= k
    idx["f"][later] = 2
    idx["o"][later] -= k
    two["index"] = idx.tobytes()
    store2 = _write_store(tmp_path / "two.ovlStore", two)
    for bgn, end in ranges + [(8, 8), (9, 12)]:
        cp, got = _read_store(host_check, store2, bgn, end, tmp_path)
        assert cp.returncode == 0, cp.stderr
        assert np.array_equal(got, rec[(rec["a"] >= bgn) & (rec["a"] <= end)]), (bgn, end)


def test_store_reader_refuses_damaged_stores(host_check, tmp_path):
    files, rec, _ = _store_fixture()
    info = np.frombuffer(files["info"], dtype="<u8")
    idt = np.dtype([("a", "<u4"), ("f", "<u4"), ("o", "<u4"), ("n", "<u4"), ("id", "<u8")])
    idx = np.frombuffer(files["index"], dtype=idt)

    def with_info(k, v):
        i = info.copy()
        i[k] = v
        return i.tobytes()

    def with_index(row, field, v):
        i = idx.copy()
        i[field][row] = v
        return i.tobytes()

    full = int(np.nonzero(idx["n"] > 0)[0][2])
    later = int(np.nonzero(idx["n"] > 0)[0][5])           # a record the stream reaches later
    cases = {
        "no info": {"info": None},
        "short info": {"info": files["info"][:40]},
        "incomplete": {"info": with_info(0, 0x50564f3a756e6163)},
        "magic": {"info": with_info(0, 0x1234)},
        "version": {"info": with_info(1, 3)},
        "bits": {"info": with_info(7, 24)},
        "no index": {"index": None},
        "index cut": {"index": files["index"][:-7]},
        "data cut": {"0001": files["0001"][:len(files["0001"]) // 2]},
        "data ragged": {"0001": files["0001"][:-3]},
        "no data": {"0001": None},
        "fileno": {"index": with_index(full, "f", 9)},
        "fileno 0": {"index": with_index(full, "f", 0)},
        "offset": {"index": with_index(full, "o", 1 << 30)},
        "count": {"index": with_index(full, "n", 1 << 31)},
        "a_iid": {"index": with_index(full, "a", full - 1)},
        "later offset": {"index": with_index(later, "o", int(idx["o"][later]) + 1)},
        "later fileno": {"index": with_index(later, "f", 2)},
        "files": {"info": with_info(6, 0)},
    }
    for name, change in cases.items():
        f = dict(files)
        for k, v in change.items():
            if v is None:
                del f[k]
            else:
                f[k] = v
        store = _write_store(tmp_path / (name.replace(" ", "_") + ".ovlStore"), f)
        cp, _ = _read_store(host_check, store, full, 0xFFFFFFFF, tmp_path)
        assert cp.returncode == 2 and cp.stderr.startswith("error: "), (name, cp.returncode,
                                                                        cp.stderr[-400:])
    # junk of the right sizes: any answer but a fault
    rng = np.random.default_rng(2)
    for k in range(6):
        f = dict(files)
        f["index"] = rng.integers(0, 256, len(files["index"]), dtype=np.uint8).tobytes() if k % 2 \
            else files["index"]
        f["0001"] = rng.integers(0, 256, len(files["0001"]), dtype=np.uint8).tobytes()
        store = _write_store(tmp_path / f"junk{k}.ovlStore", f)
        cp, _ = _read_store(host_check, store, 1, 0xFFFFFFFF, tmp_path)
        assert cp.returncode in (0, 2), (k, cp.returncode, cp.stderr[-400:])
