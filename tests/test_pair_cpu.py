"""overlapPair's host side, with no GPU: the Python restatement against the reference's
fixtures, its aligner against the quadratic DP, the arithmetic, the argument line, the .ovb
reader under sanitizers, and MHAP records -> overlaps against the reference's mhapConvert."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle
import pair_restate as PR
from canu_amd import pair
from canu_amd.mhap import MHAP_DTYPE, format_line, to_overlaps
from canu_amd.overlap_in_core import RECORD_DTYPE, write_ovb
from canu_amd.synth import ReadSet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.mark.parametrize("name", PR.FIXTURES)
def test_restatement_equals_reference(name):
    """Pins tests/pair_restate.py to the reference overlapPair: every record, every counter."""
    rs, inp, want, counters, args = PR.golden(name)
    o = PR.parse_args(args)
    got, st = PR.realign(inp, PR.reads_dict(rs), o["erate"], o["min_len"], o["partial"],
                         o["invert"])
    assert got.shape == want.shape
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (name, int(bad[0]), PR.unpack(got[bad[0]]), PR.unpack(want[bad[0]]))
    assert st == counters


def test_fixtures_cover_the_cases():
    """What the fixtures are for shows in the reference's own counters."""
    c = {n: PR.golden(n)[3] for n in PR.FIXTURES}
    assert c["b"]["nPartial"] > 0 and c["b"]["nExt5a"] == 0
    for n in ("a", "c", "d"):
        assert all(c[n][k] > 0 for k in ("nSkipped", "nPassed", "nFailed", "nFailExt",
                                         "nDovetail", "nExt5a", "nExt3a", "nExt5b", "nExt3b")), n
        assert c[n]["nFailExtA"] > c[n]["nFailExt"]          # one side failing only
    rs, inp, out, _, _ = PR.golden("d")
    assert (inp["w0"] >> np.uint64(54) & np.uint64(1)).any()     # flipped pairs
    assert b"N" in rs.bases.tobytes()


def test_bit_vector_equals_quadratic_dp():
    rng = np.random.default_rng(77)
    n_over = 0
    for case in range(400):
        small = case % 2 == 0                     # the brute-force check below is O(m n^3)
        m = int(rng.integers(1, 10 if small else 40))
        n = int(rng.integers(1, 20 if small else 60))
        alpha = b"ACGTN" if case % 3 else b"AC"
        q = bytes(alpha[i] for i in rng.integers(0, len(alpha), m))
        if case % 4 < 2:
            s = int(rng.integers(0, max(1, n - m)))
            t = bytearray(bytes(alpha[i] for i in rng.integers(0, len(alpha), n)))
            t[s:s + m] = q
            for p in rng.integers(0, len(t), int(rng.integers(0, 6))):
                t[p] = alpha[int(rng.integers(0, len(alpha)))]
            t = bytes(t)
        else:
            t = bytes(alpha[i] for i in rng.integers(0, len(alpha), n))
        for hin in (0, 1):
            assert PR.bottom_row(q, t, hin) == PR.bottom_row_dp(q, t, hin), (q, t, hin)
        k = int(rng.integers(0, m + 2))
        a = PR.infix_align(q, t, k)
        assert a == PR.infix_align(q, t, k, row=PR.bottom_row_dp)
        assert PR.global_align(q, t, k) == PR.global_align(q, t, k, row=PR.bottom_row_dp)
        n_over += a is None
        if a is not None and small:
            best, s, e = a
            # the closed definition, by brute force over every substring
            ed = lambda x, y: PR.bottom_row_dp(x, y, 1)[-1]
            assert best == min(ed(q, t[i:j + 1]) for j in range(len(t)) for i in range(j + 1))
            assert e == min(j for j in range(len(t))
                            if min(ed(q, t[i:j + 1]) for i in range(j + 1)) == best)
            assert s == min(i for i in range(e + 1) if ed(q, t[i:e + 1]) == best)
    assert 20 < n_over < 380


def test_aligner_ties_and_limits():
    assert PR.infix_align(b"AAAA", b"AAAAAAAA", 0) == (0, 0, 3)          # every column ties
    assert PR.infix_align(b"ACGACG", b"ACGACGACGACG", 0) == (0, 0, 5)
    assert PR.infix_align(b"ACGT", b"TTACGATT", 1) == (1, 2, 4)
    assert PR.infix_align(b"ACGT", b"TTACGATT", 0) is None               # best == k + 1
    assert PR.infix_align(b"NN", b"ANNA", 0) == (0, 1, 2)
    assert PR.infix_align(b"AN", b"AAAA", 0) is None                     # N equals only N
    assert PR.global_align(b"ACGT", b"AGT", 1) == 1
    assert PR.global_align(b"ACGT", b"AGT", 0) is None


def test_max_edit_and_align_len():
    """maxEdit = (int32)ceil(max(q, t) * erate * 1.1), the products in double, left to right:
    2000 * 0.045 * 1.1 is 99.00000000000001 there, not 99."""
    assert PR.max_edit(1000, 2000, 0.045) == 100
    assert PR.max_edit(10000, 11000, 0.30) == 3631
    assert PR.max_edit(2500, 3000, 0.06) == 199
    assert PR.max_edit(0, 1500, 0.144) == 238
    assert PR.max_edit(3, 2, 0.12) == 1
    assert PR.max_edit(500, 100, 0.0) == 0
    assert PR.align_len(1000, 1003, 7) == 1005
    assert PR.align_len(10, 11, 0) == 10
    assert PR.encode_evalue(0.0) == 0 and PR.encode_evalue(0.12344) == 1234
    assert PR.encode_evalue(0.12345) == 1235
    assert PR.encode_evalue(0.4095) == 4095 and PR.encode_evalue(0.40949) == 4095
    assert PR.encode_evalue(0.5) == 4095


def test_swap_ids_and_record_layout():
    r = np.array([PR.make_record(7, 9, 10, 20, 30, 40, flipped=1, span=123)], dtype=RECORD_DTYPE)
    o = PR.unpack(r[0])
    assert (o["ahg5"], o["ahg3"], o["bhg5"], o["bhg3"], o["flipped"]) == (10, 20, 30, 40, 1)
    s = PR.swap_ids(o)
    assert (s["a"], s["b"], s["ahg5"], s["ahg3"], s["bhg5"], s["bhg3"]) == (9, 7, 40, 30, 20, 10)
    o["flipped"] = 0
    s = PR.swap_ids(o)
    assert (s["ahg5"], s["ahg3"], s["bhg5"], s["bhg3"]) == (30, 40, 10, 20)
    assert PR.pack(PR.unpack(r[0])) == tuple(r[0])


def test_parse_canu_line():
    """mhap.sh's line (OverlapMhap.pm:524-534) for the three stages."""
    line = ("-G ../asm.gkpStore -O ./results/000001.mhap.ovb -o ./results/000001.WORKING.ovb "
            "-partial -len 500 -erate 0.3 -memory 13 -t 4").split()
    P, job = pair.parse_overlapPair_args(line)
    assert P == pair.PairParameters(0.3, 500, True, False)
    assert job["gkp"] == "../asm.gkpStore" and job["ovl"] == "./results/000001.mhap.ovb"
    assert job["out"] == "./results/000001.WORKING.ovb"
    assert (job["memory"], job["threads"]) == (13, 4)
    P, job = pair.parse_overlapPair_args(
        "-G g -O i -o o -len 500 -erate 0.045 -memory 6 -t 8".split())
    assert P == pair.PairParameters(0.045, 500, False, False)
    P, job = pair.parse_overlapPair_args("-G g -O i -o o -invert -b 3 -e 9".split())
    assert P.invert and P.max_erate == 0.12 and P.min_overlap_length == 0
    assert (job["bgn"], job["end"]) == (3, 9)
    for bad in ("-O i -o o", "-G g -O i", "-G g -O i -o o -x", "-G g -O i -o o -len"):
        with pytest.raises(ValueError):
            pair.parse_overlapPair_args(bad.split())


def test_report_final_text():
    c = PR.golden("a")[3]
    txt = pair.report_final(c)
    assert f" -- {c['nPassed'] + c['nFailed']} overlaps processed.\n" in txt
    assert f" -- {c['nExt5a']}/{c['nExt3a']} A read dovetail extensions\n" in txt
    assert PR.parse_report(txt) == c


def test_library_exports_and_parameter_checks(built):
    lib = pair.load_library()
    assert not [e for e in pair.EXPORTS if not hasattr(lib, e)]
    assert lib.pair_abi_version() == pair.ABI_VERSION
    p = pair._Params()
    lib.pair_params_init(p)
    assert (p.max_erate, p.min_overlap_length, p.partial, p.invert) == (0.12, 1, 0, 0)
    with pytest.raises(pair.PairError) as e:
        pair.OverlapPair(pair.PairParameters(min_overlap_length=0))
    assert e.value.code == -2
    with pytest.raises(pair.PairError):
        pair.OverlapPair(pair.PairParameters(max_erate=-1.0))


# --------------------------------------------------------------------------- the .ovb reader

@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """tests/pair_host_check.cpp under AddressSanitizer and UBSan, a program of its own."""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no C++ compiler"
    exe = str(tmp_path_factory.mktemp("pair_host") / "pair_host_check")
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "pair_host_check.cpp")], check=True, timeout=300)
    return exe


def _read(exe, path, tmp_path):
    out = str(tmp_path / "rec.bin")
    cp = subprocess.run([exe, "read", path, out], capture_output=True, text=True, timeout=120)
    return cp, (np.fromfile(out, dtype=RECORD_DTYPE) if cp.returncode == 0 else None)


def test_reader_selfcheck(host_check, tmp_path):
    cp = subprocess.run([host_check, "selfcheck", str(tmp_path)], capture_output=True, text=True,
                        timeout=300)
    assert cp.returncode == 0, cp.stdout + cp.stderr
    assert "pair_host_check ok" in cp.stdout


def test_reader_reads_the_reference_file(host_check, tmp_path):
    """basic_ref.ovb was written by the reference overlapInCore: really compressed blocks."""
    ref = os.path.join(GOLDEN, "basic_ref.ovb")
    cp, got = _read(host_check, ref, tmp_path)
    assert cp.returncode == 0, cp.stderr
    assert os.path.getsize(ref) < 24 * got.shape[0], "the fixture is not compressed"
    # the reference's own per-read counts of the same file
    counts = np.fromfile(os.path.join(GOLDEN, "basic_ref.counts"), dtype="<u4")
    opr = np.bincount(np.concatenate([got["a"], got["b"]]), minlength=int(counts[0]))
    assert counts[0] == opr.shape[0] and np.array_equal(counts[1:], opr)
    if oracle.reference_available():
        assert np.array_equal(got, oracle.read_ovb_reference(ref))


def test_reader_reads_the_projects_writer(host_check, tmp_path, built):
    _, inp, out, _, _ = PR.golden("a")
    rec = np.concatenate([inp, out] * 80)                     # 48,000 records: two blocks
    p = str(tmp_path / "ours.ovb")
    write_ovb(rec, p)
    cp, got = _read(host_check, p, tmp_path)
    assert cp.returncode == 0, cp.stderr
    assert np.array_equal(got, rec)
    write_ovb(rec[:0], p)
    cp, got = _read(host_check, p, tmp_path)
    assert cp.returncode == 0 and got.shape[0] == 0


def test_reader_refuses_damaged_files(host_check, tmp_path):
    ref = os.path.join(GOLDEN, "basic_ref.ovb")
    cp = subprocess.run([host_check, "damage", ref, str(tmp_path)], capture_output=True,
                        text=True, timeout=300)
    assert cp.returncode == 0, cp.stdout + cp.stderr
    assert "pair_host_check ok" in cp.stdout
    raw = open(ref, "rb").read()
    for name, data in (("cut", raw[:len(raw) // 2]), ("len", b"\xff" * 8 + raw[8:]),
                       ("junk", raw[:8] + bytes(len(raw) - 8))):
        p = str(tmp_path / f"{name}.ovb")
        open(p, "wb").write(data)
        cp, _ = _read(host_check, p, tmp_path)
        assert cp.returncode == 2 and cp.stderr.startswith("error: block 0"), (name, cp.stderr)
    cp, _ = _read(host_check, str(tmp_path / "absent.ovb"), tmp_path)
    assert cp.returncode == 2 and "can't open" in cp.stderr


# ------------------------------------------------------------------- MHAP records -> overlaps

def _mhap_records():
    rows = [  # a  b  erate      a_bgn a_end a_len o  b_bgn b_end b_len
        (5, 2, 0.0452341, 10, 900, 1000, 0, 0, 880, 1200),
        (5, 3, 0.1234565, 0, 1000, 1000, 1, 100, 1100, 1300),
        (6, 1, 0.4099999, 250, 990, 1000, 1, 7, 700, 900),
        (6, 6, 0.01, 0, 10, 1000, 0, 0, 10, 1000),           # a == b: left out
        (7, 4, 0.0000004, 1, 2, 1000, 0, 998, 999, 1000),
        (8, 1, 0.3, 0, 1000, 1000, 1, 0, 900, 900),
    ]
    rec = np.zeros(len(rows), dtype=MHAP_DTYPE)
    for i, r in enumerate(rows):
        (rec[i]["a"], rec[i]["b"], rec[i]["erate"], rec[i]["a_bgn"], rec[i]["a_end"],
         rec[i]["a_len"], rec[i]["o"], rec[i]["b_bgn"], rec[i]["b_end"], rec[i]["b_len"]) = r
        rec[i]["raw"] = 100.0 + i
    lens = np.array([900, 1200, 1300, 1000, 1000, 1000, 1000, 1000], dtype=np.uint32)
    rng = np.random.default_rng(5)
    offs = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.uint64)
    rs = ReadSet(bases=np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(lens.sum()))],
                 offsets=offs, lengths=lens, first_iid=1)
    return rec, rs


def test_to_overlaps_by_hand():
    rec, rs = _mhap_records()
    got = to_overlaps(rec, rs)
    assert got.shape[0] == 5 and got["a"].tolist() == [5, 5, 6, 7, 8]
    o = [PR.unpack(g) for g in got]
    assert (o[0]["ahg5"], o[0]["ahg3"], o[0]["bhg5"], o[0]["bhg3"], o[0]["flipped"]) == \
        (10, 100, 0, 320, 0)
    assert (o[1]["ahg5"], o[1]["ahg3"], o[1]["bhg5"], o[1]["bhg3"], o[1]["flipped"]) == \
        (0, 0, 200, 100, 1)                                   # flipped: the B hangs swap
    assert o[0]["evalue"] == 452 and o[1]["evalue"] == 1235   # 0.045234, 0.123457 (half up)
    assert o[2]["evalue"] == 4095 and o[3]["evalue"] == 0
    assert all(x["forOBT"] and x["forDUP"] and x["forUTG"] for x in o)
    bad = rec[:1].copy()
    bad["a_len"] = 1100                                       # longer than the stored read
    bad["a_end"] = 950
    bad["a_bgn"] = 900
    with pytest.raises(ValueError, match="INVALID OVERLAP"):
        to_overlaps(bad, rs)


@pytest.mark.skipif(not oracle.mhap_convert_available(),
                    reason="oracle/_ref/mhapConvert is not built")
def test_to_overlaps_equals_mhapConvert(tmp_path):
    rec, rs = _mhap_records()
    for hash_base, num_hash, query_base in ((1, 0, 1), (1, 4, 5)):
        p = str(tmp_path / "in.mhap")
        with open(p, "w") as f:
            for r in rec:
                f.write(format_line(r, hash_base, num_hash, query_base) + "\n")
        want = oracle.mhap_convert(rs, p, hash_base, num_hash, query_base)
        got = to_overlaps(rec, rs, hash_base, num_hash, query_base)
        assert np.array_equal(got, want), (hash_base, num_hash, query_base)
