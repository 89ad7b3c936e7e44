"""The host arithmetic of the MHAP stage (canu_amd/csrc/mhap_host.h), with no GPU: what
tests/mhap_host_check.cpp prints, against oracle/mhap_jar.py where that restates the same thing
and against hand-computed cases otherwise."""
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import mhap_jar as M
from canu_amd import mhap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """tests/mhap_host_check.cpp under AddressSanitizer and UBSan, a program of its own."""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no C++ compiler"
    exe = str(tmp_path_factory.mktemp("mhap_host") / "mhap_host_check")
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "mhap_host_check.cpp")], check=True, timeout=300)
    return exe


def _run(exe, *args, stdin=None):
    cp = subprocess.run([exe, *[a if isinstance(a, str) else repr(a) for a in args]], input=stdin,
                        capture_output=True, text=True, timeout=120)
    assert cp.returncode == 0, cp.stderr
    return cp.stdout.splitlines()


def _ints(lines):
    return [[int(v) for v in ln.split()] for ln in lines]


def _dbits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _identity(J: float, kk: int) -> float:
    """BottomOverlapSketch.jaccardToIdentity as oracle/mhap_jar.py overlap_info writes it."""
    if J > 0.0:
        return math.exp(-((-1.0 / kk) * math.log(2.0 * J / (1.0 + J))))
    return 0.0


def test_bloom_plan_is_guavas(host_check):
    expected = [0, 1, 2, 7, 1000, 123457]
    got = _ints(_run(host_check, "bloom", *expected))
    for n, (words, bits, k) in zip(expected, got):
        b = M.GuavaBloom(n, 1e-5)
        assert (words, bits, k) == (b.words.shape[0], b.bit_size, b.k), n
    assert got[0] == got[1] == [1, 64, 16]               # 0 is read as 1: 23 bits, round(15.9)
    assert got[4] == [375, 24000, 17]


def _table_lines():
    """About 40 16-mers with both strands written (as canu's -f file has them), graded fractions;
    a key written again with another fraction, fractions below the cutoff, lower-case lines."""
    rng = np.random.default_rng(41)
    comp = str.maketrans("ACGT", "TGCA")
    km, fr = [], []
    for j in range(20):
        m = "".join(rng.choice(list("ACGT"), 16))
        f = 5e-6 * (1.5 ** (j % 12))                    # j = 0, 1, 12, 13: below the 1e-5 cutoff
        km += [m, m.translate(comp)[::-1]]
        fr += [f, f]
    km += [km[6], km[9].lower(), km[0], "acgtacgtacgtacga"]
    fr += [3.1e-4, 7.7e-5, 2e-3, 4.4e-5]                # later lines replace; km[0] now passes
    return km, fr


@pytest.mark.parametrize("no_rc", [False, True])
@pytest.mark.parametrize("noise", [0, 1, 2])
def test_frequency_table_equals_frequency_counts(host_check, no_rc, noise):
    """Key set and scaledIdf (the doubles' bytes) of FrequencyCounts, the Bloom words of its
    filter, and every key found by a probe with the slot hash the kernels use."""
    km, fr = _table_lines()
    expected = 57
    p = M.default_params(repeat_idf_scale=10.0, filter_threshold=1e-5, no_rc=no_rc,
                         supress_noise=noise)
    fc = M.FrequencyCounts(km, fr, p, expected=expected)
    out = _run(host_check, "table", 16, int(not no_rc), p["repeat_weight"], p["repeat_idf_scale"],
               p["filter_threshold"], noise, expected,
               stdin="".join(f"{k} {f!r}\n" for k, f in zip(km, fr)))
    nslots, mask = map(int, out[0].split()[1:])
    keys = [ln.split()[1:] for ln in out if ln.startswith("key ")]
    assert nslots == mask + 1 >= 2 * len(keys) + 1 and nslots & mask == 0
    # 20 pairs, 4 of them below the cutoff; km[0]'s later line passes; the lower-case lines are
    # keys of their own, but with both strands a lower-case line hashes as its (upper-case, so
    # smaller) reverse complement km[8]: the pair's own key where km[8] < km[9]
    assert len(fc.counts) == (35 if no_rc else 18 + (km[8] > km[9]))
    assert sorted(int(k, 16) for k, _, _ in keys) == sorted(k & M.M64 for k in fc.counts)
    for k, sidf, found in keys:
        key = int(k, 16)
        key -= (key >> 63) << 64                            # signed, as Java's long
        assert int(sidf, 16) == _dbits(fc.scaled_idf(key)), k
        assert found == "1"
    nwords, bits, bk = map(int, next(ln for ln in out if ln.startswith("bloom ")).split()[1:])
    words = [int(ln.split()[1], 16) for ln in out if ln.startswith("word ")]
    if noise == 1:
        assert (nwords, bits, bk) == (fc.valid.words.shape[0], fc.valid.bit_size, fc.valid.k)
        assert words == [int(w) for w in fc.valid.words] and any(words)
    else:
        assert (nwords, words) == (0, [])                   # 2 builds a filter nobody reads


def test_canonical_key_is_the_smaller_strings_hash(host_check):
    kms = ["AAAAAAAAAAAAAAAC", "GTTTTTTTTTTTTTTT", "acgtacgtacgtacga", "ACGTNRYKMACGTACG"]
    for do_rc in (0, 1):
        got = [int(x, 16) for x in _run(host_check, "key", do_rc, *kms)]
        assert got == [M.seq_hashes_long(k.encode(), 16, bool(do_rc))[0] & M.M64 for k in kms]
    assert got[0] == got[1]                                 # reverse complements share a key


@pytest.mark.parametrize("S,kk,thr", [(1, 12, 0.78), (7, 12, 0.78), (64, 18, 0.8), (5, 12, 0.0)])
def test_acceptance_bits(host_check, S, kk, thr):
    out = _run(host_check, "accept", S, kk, thr)
    assert int(out[0]) == (1 if thr <= 0 else 0)            # pass_empty: identity 0 >= threshold
    words = [int(x, 16) for x in out[1:]]
    assert len(words) == ((S + 1) ** 2 + 31) // 32
    for n in range(S + 1):
        for i in range(S + 1):
            b = n * (S + 1) + i
            want = 1 <= n and i <= n and _identity(i / float(n), kk) >= thr
            assert (words[b >> 5] >> (b & 31)) & 1 == int(want), (n, i)
    if thr > 0:
        assert any(words) and not (words[(S + 1) >> 5] >> ((S + 1) & 31)) & 1   # (1, 0): J = 0


def test_weighting_mode_and_bitslice_weight(host_check):
    cases = [(rw, t, sc) for rw in (-1.0, 0.0, 0.9, 1.0) for t in (0, 1)
             for sc in (1.0, 2.5, 3.0, 10.0)]
    got = _ints(_run(host_check, "weight", *[v for c in cases for v in c]))
    for (rw, t, sc), (mode, w) in zip(cases, got):
        want = 0 if rw < 0 else 1 if (t and rw < 1.0) else 2   # W_ONE, W_TFIDF, W_COUNT
        assert mode == want, (rw, t)
        assert w == (max(1, M.java_round(sc)) if mode == 1 else 1), (rw, t, sc)
    assert dict(zip(cases, got))[(0.9, 1, 2.5)] == [1, 3]      # Java rounds half up


@pytest.mark.parametrize("k,kk,min_olap", [(16, 12, 500), (4, 18, 10)])
@pytest.mark.parametrize("no_rc", [0, 1])
def test_strands_in_use(host_check, k, kk, min_olap, no_rc):
    lens = [0, k - 1, k, min_olap - 1, min_olap, kk - 1, kk, 3000]
    (used, min_use, *sids), = _ints(_run(host_check, "strands", k, kk, min_olap, no_rc, 0,
                                         len(lens), *lens))
    assert min_use == max(min_olap, k)
    ok = [r for r, L in enumerate(lens) if L >= min_olap and L >= k and L >= kk]
    assert used == len(ok) and 0 < len(ok) < len(lens)
    assert sids == [2 * r + s for r in ok for s in ((0,) if no_rc else (0, 1))]
    # a range inside the reads: r0 = 2, three reads
    (used2, _, *sids2), = _ints(_run(host_check, "strands", k, kk, min_olap, no_rc, 2, 3, *lens))
    assert sids2 == [s for s in sids if 2 <= s >> 1 < 5] and used2 == len({s >> 1 for s in sids2})


def test_sketch_batch_plan(host_check):
    k = 16
    counts = [4, 4, 4, 0, 25, 1, 1, 1, 1]
    lens = [c + k - 1 if c else 7 for c in counts]          # 7 < k: no k-mer
    got = _ints(_run(host_check, "batches", k, 10, 3, *lens))
    # 4 + 4 fit 10 and a third 4 does not; 4 + 0 and then 25 does not; 25 alone, over the budget;
    # three 1s are the most strands a batch takes; the last 1
    assert got == [[0, 2, 8, 0, 4, 8], [2, 4, 4, 0, 4, 4], [4, 5, 25, 0, 25],
                   [5, 8, 3, 0, 1, 2, 3], [8, 9, 1, 0, 1]]
    at = 0
    for a, b, tot, *koff in got:
        assert a == at and b > a and len(koff) == b - a + 1
        assert koff == [sum(counts[a:a + i]) for i in range(b - a + 1)] and koff[-1] == tot
        at = b
    assert at == len(counts)                                # every strand once, in order
    one, = _ints(_run(host_check, "batches", k, 1 << 29, 1 << 20, *lens))
    assert one[:3] == [0, len(counts), sum(counts)]
    assert _run(host_check, "batches", k, 10, 3) == []


def test_index_and_compare_sizes(host_check):
    H = [1, 2, 128, 512, 1024]
    assert _ints(_run(host_check, "sizes", *[v for h in H for v in ("end_bit", h)])) == \
        [[33], [34], [40], [42], [43]]                      # bits of j <= H above the 32 of a value
    for h, (e,) in zip(H, [[33], [34], [40], [42], [43]]):
        assert (h << 32) < (1 << e) <= (h << 33)
    assert _ints(_run(host_check, "sizes", "initial", 1, "initial", 1024, "initial", 1025,
                      "grown", 0, "grown", 65536, "grown", 1000003)) == \
        [[65536], [65536], [65600], [1024], [65536 + 16384 + 1024], [1000003 + 250000 + 1024]]
    assert _ints(_run(host_check, "sizes", "blocks", 0, "blocks", 1, "blocks", 16384,
                      "blocks", 16385, "rec", 0, "rec", 5000)) == \
        [[0], [1], [16384], [16384], [1024], [5000]]
    assert _ints(_run(host_check, "sizes", "compare_lds", 1536, "compare_lds", 2048,
                      "minhash_lds", 512, "bitslice_lds", 512, "candidates_lds", 0)) == \
        [[3 * 8 * 1536 + 1024], [3 * 8 * 2048 + 1024], [24 * 4 * 512], [16 * 512], [65536]]
    assert _ints(_run(host_check, "range", 5, 10, 5, 14, 4, 14, 5, 15, 9, 8, 14, 14)) == \
        [[1], [0], [0], [0], [1]]


def test_java_fixed6(host_check):
    """The cases of test_java_arithmetic and test_library_formats_lines_like_java, and
       0.0000005       shortest decimal 5.0E-7: 7th decimal 5, half up    -> 0.000001
       0.9999995       7th decimal 5: carries through the 9s              -> 1.000000
       1e-7            0.0000001: 7th decimal 1                           -> 0.000000
       123456.7890125  7th decimal 5                                      -> 123456.789013
       -0.1234565      the magnitude rounds half up                       -> -0.123457"""
    want = {5e-7: "0.000001", 116.0: "116.000000", 0.0: "0.000000", 0.06954645004: "0.069546",
            1.0000005: "1.000001", 0.0000005: "0.000001", 0.9999995: "1.000000",
            1e-7: "0.000000", 123456.7890125: "123456.789013", -0.1234565: "-0.123457"}
    vals = list(want) + [1.0, 0.123456499999, 0.1234565, 2.5e-7]
    got = _run(host_check, "fixed6", *vals)
    for v, g in zip(vals, got):
        assert g == mhap.java_fixed6(v), v
        assert g == want.get(v, g), v
    assert got[-3:] == ["0.123456", "0.123457", "0.000000"]


def test_fetch_order_and_records(host_check):
    """Sorted by (a, b, o); IDs shifted by first_iid; erate = 1 - min(identity, 1); the line."""
    recs = [(5, 2, 1, 3, 9), (5, 2, 0, 9, 9), (3, 7, 0, 0, 0), (5, 1, 1, 4, 7), (3, 7, 1, 2, 5),
            (3, 1, 0, 1, 1)]
    out = _run(host_check, "fetch", 100, 12, *[v for r in recs for v in r])
    assert len(out) == len(recs)
    for (a, b, o, inter, n), ln in zip(sorted(recs, key=lambda r: r[:3]), out):
        rec, line = ln.split("|")
        ga, gb, go, erate, count, nline = rec.split()
        assert (int(ga), int(gb), int(go), int(count)) == (100 + a, 100 + b, o, 9)
        e = 1.0 - min(_identity(inter / float(n) if n else 0.0, 12), 1.0)
        assert int(erate, 16) == _dbits(e)
        r = np.zeros(1, dtype=mhap.MHAP_DTYPE)
        r[0] = (100 + a, 100 + b, e, float(inter), 1, 2, 3, o, 4, 5, 6, 9)
        assert line == mhap.format_line(r[0]) and int(nline) == len(line)
    assert out[0].split()[:3] == ["103", "101", "0"] and out[-1].split()[:3] == ["105", "102", "1"]


def test_argument_checks(host_check):
    ok = (16, 512, 3, 1536, 12, 0.2, 0)
    msgs = {(): "", (0, 0): "k-mer sizes must be 1..32", (4, 33): "k-mer sizes must be 1..32",
            (1, 1025): "num_hashes must be 1..1024", (3, 2049): "ordered_sketch must be 1..2048",
            (2, 0): "min_matches must be >= 1", (5, -1.5): "--max-shift must be >= -1",
            (5, math.nan): "--max-shift must be >= -1",
            (6, -1): "--min-store-length must be >= 0"}
    for edit, msg in msgs.items():
        p = list(ok)
        if edit:
            p[edit[0]] = edit[1]
        assert _run(host_check, "params", *p) == [msg], edit
    assert _run(host_check, "weighting", 3.0, 0) == ["", "null weighting"]
    assert _run(host_check, "weighting", 0.5, 0)[0] == "The minimum repeat idf scale must be >=1.0."
    assert _run(host_check, "weighting", 3.0, 3)[0] == "Unknown removeUnique option 3."
