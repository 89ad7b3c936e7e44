"""alignGFA on the GPU (libcanu_gfa.so and canu_amd/bin/alignGFA): the reference's output file and
stderr, plain and -V, on the fixtures in all three modes, and block / stripe / leaf boundaries,
thresholds, path shapes, windows, batches and error returns against the Python restatement
(tests/gfa_restate.py, itself pinned to the reference by tests/test_gfa_cpu.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import gfa_restate as GR
from canu_amd import align_gfa as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "canu_amd", "bin", "alignGFA")
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _rand(rng, n):
    return _ACGT[rng.integers(0, 4, n)].tobytes()


def _subs(rng, seq, n, lo=0, hi=None):
    """n substitutions at distinct, evenly spread places of seq[lo:hi]."""
    out = bytearray(seq)
    hi = len(seq) if hi is None else hi
    for p in np.linspace(lo + 3, hi - 4, n).astype(int):
        out[p] = b"ACGT"[(b"ACGT".index(out[p]) + int(rng.integers(1, 4))) % 4]
    return bytes(out)


def _links(spec):
    return np.array(spec, dtype=G.LINK_DTYPE).reshape(-1)


LINK_FIELDS = ("max_edit", "a_len", "b_len", "abgn_b", "bend_b", "dist_b", "bend", "abgn_a", "dist_a",
               "abgn", "dist_f", "align_len")


def _check_links(tigs, spec, params=None):
    """The library against the restatement: every coordinate and distance of every step, the
    CIGAR, and the leaves and splits of the path.  -> (results, cigars, restatement, stats)."""
    links = _links(spec)
    g = G.AlignGFA(params)
    g.load_tigs(G.SET_T, tigs)
    res, runs = g.check_links(links)
    st = g.stats()
    g.close()
    log = GR.new_log()
    seqs = [t or b"" for t in tigs]
    want, cigars = [], []
    for i, l in enumerate(links):
        link = {"Aid": int(l["a_id"]), "Afwd": bool(l["a_fwd"]), "Bid": int(l["b_id"]),
                "Bfwd": bool(l["b_fwd"]), "cigar": None,
                "lengths": (int(l["a_align"]), int(l["b_align"]), int(l["align"]))}
        w = GR.check_link(link, seqs, log, None)
        want.append(w)
        r = res[i]
        for f in LINK_FIELDS:
            assert int(r[f]) == int(w[f]), (i, f, int(r[f]), int(w[f]))
        assert bool(r["success"]) == w["success"], i
        got = G.cigar_text(runs[int(r["run_off"]):int(r["run_off"]) + int(r["n_runs"])])
        cigars.append(got if r["success"] else None)
        assert cigars[-1] == w["cigar"], (i, cigars[-1], w["cigar"])
        assert (int(r["n_leaves"]), int(r["n_splits"])) == (w["leaf"], w["split"]), i
    assert (st["n_leaves"], st["n_splits"]) == (log["leaf"], log["split"])
    assert st["dp_cells"] == log["cells"]
    assert st["n_alignments"] == log["alignments"] == 3 * len(links)
    return res, cigars, want, st


def _overlap_pair(rng, n, a_extra=700, b_extra=900):
    """Two tigs whose ends share n exact bases."""
    o = _rand(rng, n)
    return [_rand(rng, a_extra) + o, o + _rand(rng, b_extra)]


# ------------------------------------------------------------------ the fixtures

@pytest.mark.parametrize("name", GR.FIXTURES)
@pytest.mark.parametrize("verbose", [False, True])
def test_fixture_library(name, verbose):
    """Every fixture through the library and the text helpers: the reference's bytes."""
    g = GR.golden(name)
    T = GR.store_tigs(g["gapped_T"])
    C = GR.store_tigs(g["gapped_C"]) if g["gapped_C"] is not None else None
    a = G.AlignGFA()
    out, err = G.run_program(a, g["args"] + (["-V"] if verbose else []), T, C, g["input"])
    a.close()
    assert out == (g["out_v"] if verbose else g["out"])
    assert err == (g["err_v"] if verbose else g["err"])


def _write_store(path, gapped):
    os.makedirs(path)
    tig, dat = GR.encode_tigstore(gapped)
    for ext, raw in (("tig", tig), ("dat", dat)):
        with open(os.path.join(path, "seqDB.v002." + ext), "wb") as f:
            f.write(raw)


@pytest.mark.parametrize("name", GR.FIXTURES)
def test_fixture_executable(name, tmp_path):
    """Every fixture through canu_amd/bin/alignGFA, plain and -V: the reference's files."""
    g = GR.golden(name)
    d = str(tmp_path)
    _write_store(os.path.join(d, "T.tigStore"), g["gapped_T"])
    if g["gapped_C"] is not None:
        _write_store(os.path.join(d, "C.tigStore"), g["gapped_C"])
    with open(os.path.join(d, "in"), "w") as f:
        f.write(g["input"])
    for extra, out, err in (([], g["out"], g["err"]), (["-V"], g["out_v"], g["err_v"])):
        cp = subprocess.run([CLI, *g["args"], "-t", "1", *extra], cwd=d, capture_output=True)
        assert cp.returncode == 0, cp.stderr.decode()[-2000:]
        assert cp.stderr.decode() == err
        with open(os.path.join(d, "out")) as f:
            assert f.read() == out


def test_executable_refuses(tmp_path):
    d = str(tmp_path)
    for argv in (["-G", "x"], ["-T", "T.tigStore", "2", "-i", "in"], ["-T", "T.tigStore", "0", "-i",
                 "in", "-o", "out"], ["-T", "missing.tigStore", "2", "-i", "in", "-o", "out"]):
        cp = subprocess.run([CLI, *argv], cwd=d, capture_output=True)
        assert cp.returncode == 1, argv


# ------------------------------------------------------------------ links

def test_no_links_and_one_link():
    rng = np.random.default_rng(1)
    tigs = _overlap_pair(rng, 300)
    g = G.AlignGFA()
    g.load_tigs(G.SET_T, tigs)
    res, runs = g.check_links(_links([]))
    assert res.shape == (0,) and runs.shape == (0,) and g.stats()["n_rounds"] == 0
    g.close()
    _, cigars, _, _ = _check_links(tigs, [(0, 1, 1, 1, 300, 300, 300)])
    assert cigars == ["300M"]


@pytest.mark.parametrize("n", [63, 64, 65, 4095, 4096, 4097])
def test_query_lengths(n):
    """Queries that end one row short of, on and one row past a 64-row block and a 4096-row
    stripe, in both orientations, with a few differences."""
    rng = np.random.default_rng(100 + n)
    o = _rand(rng, n)
    a, b = _rand(rng, 500) + o, _subs(rng, o, 3) + _rand(rng, 600)
    tigs = [a, b, GR.FS.revcomp(a), GR.FS.revcomp(b)]
    res, _, _, _ = _check_links(tigs, [(0, 1, 1, 1, n, n, n), (2, 0, 3, 0, n, n, n),
                                      (0, 1, 3, 0, n, n, n)])
    assert all(int(r["a_len"]) - int(r["abgn_b"]) == n for r in res)


@pytest.mark.parametrize("b_align,cols", [(14895, 16384), (14896, 16385)])
def test_boundary_row_in_lds_and_global(b_align, cols):
    """A query past 4096 rows against a target of 16384 columns (the stripe boundary row in
    LDS) and of 16385 (in the global row)."""
    rng = np.random.default_rng(7)
    o = _rand(rng, 5000)
    tigs = [_rand(rng, 300) + o, _subs(rng, o, 40) + _rand(rng, 12000)]
    res, _, _, _ = _check_links(tigs, [(0, 1, 1, 1, 5000, b_align, 5000)])
    assert int(res[0]["bend_b"]) == cols and int(res[0]["a_len"]) - int(res[0]["abgn_b"]) == 5000
    assert res[0]["success"]


@pytest.mark.parametrize("n,leaf", [(1790, True), (1800, False)])
def test_leaf_and_split(n, leaf):
    """The final alignment of n x n: the largest that is one leaf, and the first that splits.
    The path of an exact overlap is one run."""
    rng = np.random.default_rng(n)
    res, cigars, want, _ = _check_links(_overlap_pair(rng, n), [(0, 1, 1, 1, n, n, n)])
    r = res[0]
    assert (int(r["a_len"]) - int(r["abgn"]), int(r["bend"])) == (n, n)
    assert GR.FS.is_leaf(n, n) == leaf
    assert (int(r["n_splits"]) == 0) == leaf
    assert cigars == ["%dM" % n]


def test_split_with_differences():
    """A path over several levels of splits, with insertions and deletions."""
    rng = np.random.default_rng(11)
    o = _rand(rng, 6000)
    m = bytearray(_subs(rng, o, 60))
    for p in (5500, 4000, 2500, 900):
        del m[p:p + 3]
        m[p - 300:p - 300] = b"ACG"
    tigs = [_rand(rng, 400) + o, bytes(m) + _rand(rng, 800)]
    res, cigars, _, _ = _check_links(tigs, [(0, 1, 1, 1, 6000, 6000, 6000)])
    assert res[0]["success"] and int(res[0]["n_splits"]) >= 3
    assert "I" in cigars[0] and "D" in cigars[0]


@pytest.mark.parametrize("extra", [0, 1])
def test_extension_threshold(extra):
    """The extension steps at a distance equal to maxEdit, and one above it."""
    rng = np.random.default_rng(21)
    n = 500
    k = int(np.ceil(n * 0.12))
    o = _rand(rng, n)
    tigs = [_rand(rng, 800) + o, _subs(rng, o, k + extra) + _rand(rng, 800)]
    res, _, want, _ = _check_links(tigs, [(0, 1, 1, 1, n, n, n)])
    assert want[0]["max_edit"] == k
    if extra == 0:
        assert (want[0]["dist_b"], want[0]["dist_a"]) == (k, k)
    else:
        assert (want[0]["dist_b"], want[0]["dist_a"]) == (-1, -1)


@pytest.mark.parametrize("extra", [0, 1])
def test_final_threshold(extra):
    """The final alignment at a distance equal to 2 * maxEdit, and one above it: the two ends
    of 1100 bases differ in 120 or 121 places, the extensions fail, maxEdit is 60."""
    rng = np.random.default_rng(22)
    o = _rand(rng, 1100)
    tigs = [_rand(rng, 500) + o, _subs(rng, o, 120 + extra) + _rand(rng, 500)]
    res, _, want, _ = _check_links(tigs, [(0, 1, 1, 1, 1000, 1000, 500)])
    assert want[0]["max_edit"] == 60 and (want[0]["dist_b"], want[0]["dist_a"]) == (-1, -1)
    assert want[0]["success"] == (extra == 0)
    if extra == 0:
        assert want[0]["dist_f"] == 120


def test_indel_runs_at_both_ends():
    """A path that begins with a run of D and ends with a run of I."""
    rng = np.random.default_rng(23)
    cgt = np.frombuffer(b"CGT", dtype=np.uint8)
    # B begins with 30 A that A lacks (Abgn is clamped to 0), A ends with 20 A that B lacks (Bend
    # is clamped to Blen); what they share has no A near its ends, so the runs are clean
    core = cgt[rng.integers(0, 3, 40)].tobytes() + _rand(rng, 420) + cgt[rng.integers(0, 3, 40)].tobytes()
    tigs = [core + b"A" * 20, b"A" * 30 + core]
    _, cigars, want, _ = _check_links(tigs, [(0, 1, 1, 1, 600, 600, 600)])
    assert want[0]["success"] and cigars == ["30D500M20I"]


def test_n_and_nul():
    """N on a forward tig differs from the NUL a reversed N becomes; two NULs are equal."""
    rng = np.random.default_rng(24)
    o = bytearray(_rand(rng, 400))
    for p in (50, 200, 333):
        o[p] = ord("N")
    o = bytes(o)
    rc = GR.FS.revcomp
    tigs = [_rand(rng, 300) + o, o + _rand(rng, 300), rc(o + _rand(rng, 300)),
            rc(_rand(rng, 300) + o)]
    res, _, want, _ = _check_links(tigs, [(0, 1, 1, 1, 400, 400, 400), (0, 1, 2, 0, 400, 400, 400),
                                          (3, 0, 2, 0, 400, 400, 400)])
    assert [w["dist_f"] for w in want] == [0, 3, 0]


def test_clamps_and_longer_query():
    """AalignLen beyond A (Abgn clamped to 0), 1.1 x BalignLen beyond B (Bend clamped), and a
    query longer than its target in extend A."""
    rng = np.random.default_rng(25)
    gnm = _rand(rng, 4000)
    tigs = [gnm[2600:3000], gnm[2500:3500], gnm[0:3000], gnm[2500:3020]]
    res, _, want, _ = _check_links(tigs, [(0, 1, 1, 1, 500, 500, 500), (2, 1, 3, 1, 500, 500, 500)])
    assert int(res[0]["abgn_b"]) == 0 and int(res[1]["bend_b"]) == 520
    assert int(res[0]["bend"]) > int(res[0]["a_len"]) - int(res[0]["abgn_a"])


def test_batches_and_determinism():
    """2,000 short links under a budget of 1 MiB run in several batches, with the output of one
    batch; two equal runs are equal."""
    job = G.synth_graph(seed=5, n_links=2000, n_records=0, tig_len=600, overlap=200,
                        error_rate=0.02)
    outs = []
    for budget in (0, 1 << 20, 1 << 20):
        g = G.AlignGFA(G.GfaParameters(hbm_budget=budget))
        g.load_tigs(G.SET_T, job["utgs"])
        res, runs = g.check_links(job["links"])
        outs.append((res, runs, g.stats()["n_batches"]))
        g.close()
    assert outs[0][2] == 1 and outs[1][2] > 1
    for res, runs, _ in outs[1:]:
        assert np.array_equal(res, outs[0][0]) and np.array_equal(runs, outs[0][1])
    assert 0 < int(outs[0][0]["success"].sum()) < 2000
    # a sample against the restatement
    seqs = job["utgs"]
    log = GR.new_log()
    for i in range(0, 2000, 97):
        l, r = job["links"][i], outs[0][0][i]
        link = {"Aid": int(l["a_id"]), "Afwd": bool(l["a_fwd"]), "Bid": int(l["b_id"]),
                "Bfwd": bool(l["b_fwd"]), "cigar": "%dM" % l["align"]}
        w = GR.check_link(link, seqs, log, None)
        got = G.cigar_text(outs[0][1][int(r["run_off"]):int(r["run_off"]) + int(r["n_runs"])])
        assert (got if r["success"] else None) == w["cigar"], i


# ------------------------------------------------------------------ placements

def _check_records(utgs, ctgs, spec):
    recs = np.array(spec, dtype=G.RECORD_DTYPE).reshape(-1)
    g = G.AlignGFA()
    g.load_tigs(G.SET_T, utgs)
    g.load_tigs(G.SET_C, ctgs)
    res, tries = g.check_records(recs)
    g.close()
    log = GR.new_log()
    for i, r in enumerate(recs):
        rec = {"Aid": int(r["a_id"]), "Bid": int(r["b_id"]), "Bfwd": bool(r["b_fwd"]),
               "bgn": int(r["bgn"]), "end": int(r["end"]), "Aname": "c", "Bname": "u", "score": 0}
        ok, wt = GR.check_record(rec, ctgs, utgs, log, None)
        got = res[i]
        assert bool(got["success"]) == ok, i
        assert (int(got["bgn"]), int(got["end"])) == (rec["bgn"], rec["end"]), i
        mine = tries[int(got["try_off"]):int(got["try_off"]) + int(got["n_tries"])]
        assert len(mine) == len(wt), (i, len(mine), len(wt))
        for t, w in zip(mine, wt):
            assert int(t["record"]) == i
            for f in ("call", "b_len", "abgn", "aend", "max_edit", "dist", "outcome"):
                assert int(t[f]) == w[f], (i, f, int(t[f]), w[f])
            if w["dist"] >= 0:
                assert (int(t["nbgn"]), int(t["nend"])) == (w["nbgn"], w["nend"]), i
    return res, tries


def test_records_rounds_and_contig_ends():
    """A unitig from nowhere takes five or more rounds to ABORT; one 600 bases off takes RELAX
    rounds to its place; a window clamped at both contig ends; a reversed unitig; no records."""
    rng = np.random.default_rng(31)
    c0, c1 = _rand(rng, 6000), _rand(rng, 1000)
    utgs = [_rand(rng, 500), c0[3600:4400], c1[50:950], GR.FS.revcomp(c0[1000:2200])]
    res, tries = _check_records(utgs, [c0, c1], [(0, 0, 1, 4000, 4500), (0, 1, 1, 3000, 3800),
                                                 (1, 2, 1, 50, 950), (0, 3, 0, 1010, 2190)])
    assert not res[0]["success"] and int(res[0]["n_tries"]) >= 5
    assert int(tries[int(res[0]["try_off"]) + int(res[0]["n_tries"]) - 1]["outcome"]) == G.ABORT
    assert res[1]["success"] and (int(res[1]["bgn"]), int(res[1]["end"])) == (3600, 4400)
    t2 = tries[int(res[2]["try_off"])]
    assert (int(t2["abgn"]), int(t2["aend"])) == (0, 1000) and int(t2["outcome"]) == G.ACCEPT
    assert res[3]["success"] and (int(res[3]["bgn"]), int(res[3]["end"])) == (1000, 2200)
    r0, t0 = _check_records(utgs, [c0, c1], [])
    assert r0.shape == (0,) and t0.shape == (0,)


def test_records_49999_and_50000():
    """Fixture c's unitigs of 50,000 (LEFT / RIGHT) and 49,999 (ALL) bases, every try against
    the reference's -V log: the restatement takes ten seconds on these."""
    g = GR.golden("c")
    T, C = GR.store_tigs(g["gapped_T"]), GR.store_tigs(g["gapped_C"])
    assert sorted(len(t) for t in T) == [49999, 50000]
    a = G.AlignGFA()
    a.load_tigs(G.SET_T, T)
    a.load_tigs(G.SET_C, C)
    bed = G.parse_bed(g["input"])
    res, tries = a.check_records(bed["array"])
    a.close()
    calls = [G.CALLS[int(t["call"])] for t in tries]
    assert calls.count("ALL") >= 1 and calls.count("LEFT") >= 1 and calls.count("RIGHT") >= 1
    log = "".join(G.try_log(t, bed["records"][int(t["record"])][0],
                            bed["records"][int(t["record"])][3], len(C[0])) for t in tries)
    assert log == "".join(l + "\n" for l in g["err_v"].split("\n") if l.startswith("ALIGN"))


# ------------------------------------------------------------------ errors

def _raises(code, fn, *a):
    with pytest.raises(G.GfaError) as e:
        fn(*a)
    assert e.value.code == code, (e.value.code, str(e.value))


def test_error_returns():
    rng = np.random.default_rng(41)
    tigs = _overlap_pair(rng, 300) + [b""]
    ok = [(0, 1, 1, 1, 300, 300, 300)]
    with pytest.raises(G.GfaError) as e:
        G.AlignGFA(device=99)
    assert e.value.code == -1
    g = G.AlignGFA()
    lib = g.lib
    _raises(-7, g.check_links, _links(ok))                           # no tigs
    n = ctypes.c_uint64()
    assert lib.gfa_runs_size(g.ctx, ctypes.byref(n)) == -7
    assert lib.gfa_tries_size(g.ctx, ctypes.byref(n)) == -7
    _raises(-2, g.load_tigs, 2, tigs)                                # no such set
    _raises(-4, g.load_tigs, G.SET_T, [b"ACGTX"])                    # a byte outside ACGTN
    _raises(-4, g.load_tigs, G.SET_T, [b"acgt"])
    g.load_tigs(G.SET_T, tigs)
    _raises(-7, g.check_records, np.zeros(1, dtype=G.RECORD_DTYPE))  # no contigs
    for bad in ((3, 1, 1, 1, 300, 300, 300), (0, 1, 3, 1, 300, 300, 300),      # outside the store
                (2, 1, 1, 1, 300, 300, 300), (0, 1, 2, 1, 300, 300, 300),      # no sequence
                (0, 1, 1, 1, 0, 300, 300), (0, 1, 1, 1, 300, 0, 300),          # an empty span
                (0, 1, 1, 1, 0, 0, 0), (0, 1, 1, 1, 300, 300, -1)):            # '*'
        _raises(-4, g.check_links, _links(ok + [bad]))
    assert lib.gfa_check_links(g.ctx, None, 1, None) == -2
    assert lib.gfa_check_links(None, None, 0, None) == -2
    res, _ = g.check_links(_links(ok))                               # and it still works
    assert res[0]["success"]
    g.load_tigs(G.SET_C, [tigs[0], b""])
    for bad in ((2, 1, 1, 0, 100), (0, 3, 1, 0, 100), (1, 1, 1, 0, 0), (0, 2, 1, 0, 100),
                (0, 1, 1, -1, 100), (0, 1, 1, 0, len(tigs[0]) + 1), (0, 1, 1, 200, 100)):
        _raises(-4, g.check_records, np.array([bad], dtype=G.RECORD_DTYPE))
    g.set_params(G.GfaParameters(hbm_budget=1 << 20))
    assert lib.gfa_set_params(g.ctx, None) == -2
    g.close()
