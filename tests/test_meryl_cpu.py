"""The k-mer count's host side, with no GPU: the numpy restatement against the reference's
golden texts, estimate-mer-threshold and the Meryl.pm glue, the database files, the two
executables' host-only modes, and the sanitizer build of the host header."""
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

import meryl_numpy as MN
from canu_amd import meryl
from canu_amd.mhap import read_frequency_file
from canu_amd.overlap_in_core import read_skip_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMT = np.load(os.path.join(MN.GOLDEN, "meryl_emt.npz"))


@pytest.fixture(scope="module")
def bins(built):
    from canu_amd import build as B
    return B.MERYL_CLI_OUT, B.EMT_CLI_OUT


@pytest.mark.parametrize("name", MN.FIXTURES)
def test_numpy_restatement_equals_reference(name):
    """Pins tests/meryl_numpy.py to the reference meryl's own output, byte for byte."""
    _, k, texts, c = MN.golden(name)
    assert c.info_text() == texts["info"]
    assert c.histogram_text() == texts["histogram"]
    # the reference's build keeps every mer whatever its -L (no line of src/meryl reads
    # lowCount after the argument check), so its -Dt -n 1 lists the count-1 mers too: that is
    # low_count 1 here; from the threshold 2 on, low_count 2 gives the same bytes
    for t, want in texts["dt"].items():
        assert c.with_low(1).threshold_text(t) == want, (name, t)
        if t >= 2:
            assert c.threshold_text(t) == want, (name, t)


def test_issue_sample_semantics():
    """Fixture a: NNN removes k+2 mers of one read; low_count 2 keeps count-1 mers out of the
    kept list but in the totals and in histogram row 1."""
    rs, k, texts, c = MN.golden("a_k16")
    assert c.total == 60 * (600 - k + 1) - (k + 2)
    assert c.threshold_text(1) == texts["dt"][2] != texts["dt"][1]
    assert texts["dt"][1].count(b">1\n") == c.unique
    assert texts["histogram"].split(b"\n")[0].split(b"\t")[:2] == [b"1", b"%d" % c.unique]


@pytest.mark.parametrize("name", [str(n) for n in EMT["names"]])
def test_estimate_threshold_python(name):
    hist = EMT[f"{name}__hist"].tobytes().decode()
    for cov in EMT["coverages"]:
        cov = int(cov)
        log = []
        got = meryl.estimate_threshold(hist, cov, log)
        assert got == int(EMT[f"{name}__out_{cov}"].tobytes()), (name, cov)
        assert "\n".join(log) + "\n" == EMT[f"{name}__err_{cov}"].tobytes().decode()


def test_estimate_threshold_exits_covered():
    """The synthetic histograms take the loops' different exits (recorded in the reference's
    stderr), and one has products beyond 2^32."""
    errs = {str(n): EMT[f"{n}__err_0"].tobytes().decode() for n in EMT["names"]}
    assert "Found break in kmer coverage" in errs["syn_gap"]
    assert "No break in kmer coverage found" in errs["syn_nobreak"]
    h = meryl.load_histogram_text(EMT["syn_wrap__hist"].tobytes().decode())
    assert max(c * n for c, n in enumerate(h)) > 1 << 32
    # -c changes the answer where the coverage rules decide
    assert int(EMT["syn_ninety__out_30"].tobytes()) != int(EMT["syn_ninety__out_1"].tobytes())
    assert int(EMT["syn_jump__out_1"].tobytes()) != int(EMT["syn_jump__out_0"].tobytes())


def test_estimate_threshold_cli(bins, tmp_path):
    for name in EMT["names"]:
        hp = tmp_path / f"{name}.histogram"
        hp.write_bytes(EMT[f"{name}__hist"].tobytes())
        for cov in EMT["coverages"]:
            cov = int(cov)
            cp = subprocess.run([bins[1], "-h", str(hp), "-c", str(cov)], capture_output=True,
                                timeout=60)
            assert cp.returncode == 0, cp.stderr
            assert cp.stdout == EMT[f"{name}__out_{cov}"].tobytes(), (name, cov)
            assert cp.stderr == EMT[f"{name}__err_{cov}"].tobytes(), (name, cov)


def test_perl_glue():
    assert meryl.ovl_threshold("40\n", 1.0) == 41
    assert meryl.ovl_threshold(40, 1.5) == 61
    rows = MN.golden("b_k22")[2]["histogram"].decode()
    first = rows.split("\n")[0].split("\t")
    # the first row already covers its own fraction; a set threshold below it wins
    assert meryl.threshold_from_fractions(rows, 0, distinct=float(first[2])) == 1
    assert meryl.threshold_from_fractions(rows, 0, total=0.5) == next(
        int(r.split("\t")[0]) for r in rows.split("\n") if r and float(r.split("\t")[3]) >= 0.5)
    assert meryl.threshold_from_fractions(rows, 1, total=0.9999) == 1
    assert meryl.threshold_from_fractions(rows, 7) == 7
    # Meryl.pm:586-611 worked by hand on rows of its own layout
    hand = "1\t100\t0.5000\t0.1000\n2\t50\t0.7500\t0.2000\n5\t30\t0.9000\t0.3500\n" \
           "9\t15\t0.9750\t0.4850\n40\t5\t1.0000\t1.0000\n"
    f = meryl.threshold_from_fractions
    assert f(hand, 0, distinct=0.9) == 5             # first row with distinct >= 0.9
    assert f(hand, 0, total=0.4) == 9                # first row with total >= 0.4
    assert f(hand, 0, distinct=0.99, total=0.3) == 5     # both given: total reaches first
    assert f(hand, 0, distinct=0.7, total=0.9) == 2      # both given: distinct reaches first
    assert f(hand, 3, distinct=0.99) == 3            # the supplied threshold wins mid-scan (3 < 5)
    assert f(hand, 3, distinct=0.6) == 2             # ... unless a fraction is met before it
    assert f(hand, 50, total=1.0) == 40              # a fraction row below the supplied one
    assert f(hand, 0, distinct=2.0) == 0             # never met: unchanged


@pytest.mark.parametrize("name", MN.FIXTURES)
def test_database_round_trip(built, name, tmp_path):
    """A database written from the (mer, count) lists reopens host-only and gives the
    reference's three texts."""
    _, k, texts, c = MN.golden(name)
    p = str(tmp_path / "asm")
    MN.write_db(p, c)
    mc = meryl.MerCounter.open(p)
    assert mc.k == k
    st = mc.stats()
    assert (st["total_mers"], st["distinct_mers"], st["unique_mers"], st["largest_count"]) == \
        (c.total, c.distinct, c.unique, c.largest)
    assert np.array_equal(mc.histogram(), c.hist)
    gm, gc = mc.frequent(0)
    wm, wc = c.frequent(0)
    assert np.array_equal(gm, wm) and np.array_equal(gc, wc)
    mc.write_histogram(p + ".h", p + ".i")
    assert open(p + ".h", "rb").read() == texts["histogram"]
    assert open(p + ".i", "rb").read() == texts["info"]
    for t, want in texts["dt"].items():
        mc.write_threshold(t, p + ".dt")
        assert open(p + ".dt", "rb").read() == (want if t >= 2 else texts["dt"][2])
    # kept from count 1 on, the database gives the reference's -n 1 dump as well
    MN.write_db(p + "1", c.with_low(1))
    m1 = meryl.MerCounter.open(p + "1")
    m1.write_threshold(1, p + ".dt")
    assert open(p + ".dt", "rb").read() == texts["dt"].get(1, c.with_low(1).threshold_text(1))
    m1.close()
    # saved again by the library, the files are the ones the layout documents
    mc.save(p + "2")
    for ext in (".mcidx", ".mcdat"):
        assert open(p + "2" + ext, "rb").read() == open(p + ext, "rb").read()
    mc.close()


def test_database_damage_is_an_error(built, tmp_path):
    c = MN.golden("a_k16")[3]
    p = str(tmp_path / "asm")
    MN.write_db(p, c)
    idx, dat = open(p + ".mcidx", "rb").read(), open(p + ".mcdat", "rb").read()
    q = str(tmp_path / "bad")
    cases = [(idx[:len(idx) // 2], dat), (idx, dat[:len(dat) // 2]), (idx, dat[:-1]),
             (b"X" + idx[1:], dat), (idx, b"merylDataFile" + dat[13:]), (b"", dat)]
    for i, d in cases:
        open(q + ".mcidx", "wb").write(i)
        open(q + ".mcdat", "wb").write(d)
        with pytest.raises(meryl.MerError):
            meryl.MerCounter.open(q)
    with pytest.raises(meryl.MerError):
        meryl.MerCounter.open(str(tmp_path / "absent"))


def test_hand_offs_equal_the_files(built, tmp_path):
    """skip_kmers() is what read_skip_fasta reads from the -k file; the -f file parses with
    the MHAP stage's reader into what mhap_frequencies() hands over; its lines are Meryl.pm's."""
    _, k, texts, c = MN.golden("a_k16")
    p = str(tmp_path / "asm")
    MN.write_db(p, c)
    mc = meryl.MerCounter.open(p)
    fa = p + ".frequentMers.fasta"
    meryl.write_ovl_frequent_mers(mc, 12, fa)
    assert open(fa, "rb").read() == texts["dt"][12]
    assert meryl.skip_kmers(mc, 12) == read_skip_fasta(fa, k)

    ft = 0.0001                          # minCount = int(ft * 2 * total) = 7
    gz = p + ".frequentMers.ignore.gz"
    meryl.write_mhap_ignore(mc, ft, gz)
    total_mers = 2 * c.total
    min_count = int(ft * total_mers)
    assert min_count > 2
    mers, counts = c.frequent(min_count)
    lines = gzip.open(gz, "rt").read().split("\n")
    assert lines[0] == str(2 * int(c.hist[min_count:].sum()))
    assert len(lines) == 2 + 2 * mers.shape[0]
    s0 = c.threshold_text(min_count).decode().split("\n")[1]
    assert lines[1] == "%s\t%e" % (s0, counts[0] / total_mers)
    assert lines[2] == "%s\t%e" % (meryl.revcomp(s0), counts[0] / total_mers)
    # a minCount below the database's low_count would promise k-mers the dump does not hold
    for fn in (lambda: meryl.write_mhap_ignore(mc, 0.000005, gz + "x"),
               lambda: meryl.mhap_frequencies(mc, 0.000005)):
        with pytest.raises(meryl.MerError, match="low_count"):
            fn()
    assert not os.path.exists(gz + "x")
    MN.write_db(p + "1", c.with_low(1))
    m1 = meryl.MerCounter.open(p + "1")           # kept from 1 on: Meryl.pm's file for minCount 0
    meryl.write_mhap_ignore(m1, 0.000005, gz + "1")
    l1 = gzip.open(gz + "1", "rt").read().split("\n")
    assert l1[0] == str(2 * c.distinct) and len(l1) == 2 + 2 * c.distinct
    m1.close()
    km, fr, cnt = read_frequency_file(gz, k, with_count=True)
    hk, hf, hc = meryl.mhap_frequencies(mc, ft)
    assert km == hk and cnt == hc and np.array_equal(fr, hf)
    mc.close()


def test_meryl_cli_dumps(bins, tmp_path):
    """bin/meryl -Dh / -Dt on a saved database, with no GPU; other modes exit 1."""
    for name in ("a_k16", "c_k16", "a_k32"):
        _, k, texts, c = MN.golden(name)
        p = str(tmp_path / name)
        MN.write_db(p, c)
        cp = subprocess.run([bins[0], "-Dh", "-s", p], capture_output=True, timeout=60)
        assert cp.returncode == 0 and cp.stdout == texts["histogram"] and cp.stderr == texts["info"]
        for t, want in texts["dt"].items():
            cp = subprocess.run([bins[0], "-Dt", "-n", str(t), "-s", p], capture_output=True,
                                timeout=60)
            assert cp.returncode == 0 and cp.stdout == (want if t >= 2 else texts["dt"][2])
    for argv in (["-M", "add", "-s", p, "-s", p, "-o", p], ["-Dc", "-s", p], ["-Dp", "-s", p],
                 ["-P", "-m", "16", "-s", p], ["-Dt", "-s", p], ["-Dh", "-s", p + "absent"]):
        cp = subprocess.run([bins[0]] + argv, capture_output=True, timeout=60)
        assert cp.returncode == 1 and cp.stderr, argv
    cp = subprocess.run([bins[0], "-Dt", "-n", "1", "-s", p], capture_output=True, text=True,
                        timeout=60)
    assert cp.returncode == 0 and "below the -L 2" in cp.stderr
    cp = subprocess.run([bins[0], "--help"], capture_output=True, text=True, timeout=60)
    assert "may only LOWER" in cp.stderr


def test_library_exports_and_no_device_error(built):
    lib = meryl.load_library()
    assert not [e for e in meryl.EXPORTS if not hasattr(lib, e)]
    with pytest.raises(meryl.MerError):
        meryl.MerCounter(33)
    with pytest.raises(meryl.MerError):
        meryl.MerCounter(0)


def test_host_header_under_sanitizers(tmp_path):
    """tests/meryl_host_check.cpp, a program of its own: the database writer, reader and text
    writers under AddressSanitizer and UBSan."""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "meryl_host_check")
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "meryl_host_check.cpp")], check=True, timeout=300)
    cp = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert cp.returncode == 0, cp.stdout + cp.stderr
    assert "meryl_host_check ok" in cp.stdout
