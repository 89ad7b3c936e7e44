"""alignGFA without a GPU: the restatement (tests/gfa_restate.py) against the fixtures the
reference binary wrote (tests/golden/gfa_*.npz, tools/make_gfa_golden.py) and, where the
reference's objects exist, against the reference itself on fresh jobs; the branches the fixtures
reach; the text helpers of canu_amd.align_gfa; the refusals; the ABI; and the host code of the
executable (gfa_files.h, gfa_host.h) under the address and undefined-behaviour sanitizers, as a
stand-alone program."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import gfa_restate as GR
from canu_amd import align_gfa as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
REF_OBJ = os.path.join(ROOT, "oracle", "_ref", "obj", "fe_configure.o")
SLOW = ("c", "e")            # 50,000-row passes: some ten seconds each in Python


@pytest.fixture(scope="module")
def runs():
    """The restatement on every fixture, once: name -> (plain, -V) of (out, err, results, log).
    The slow fixtures run with -V alone; their plain stderr is the -V one less its ALIGN lines,
    which the fast fixtures show to hold."""
    got = {}
    for name in GR.FIXTURES:
        g = GR.golden(name)
        per = {}
        for verbose in ((True,) if name in SLOW else (False, True)):
            log = GR.new_log()
            out, err, res = GR.run_golden(g, verbose, log)
            per[verbose] = (out, err, res, log)
        got[name] = per
    return got


@pytest.mark.parametrize("name", GR.FIXTURES)
def test_restatement_reproduces_fixture(runs, name):
    g = GR.golden(name)
    for verbose, (out, err, _, _) in runs[name].items():
        assert out == (g["out_v"] if verbose else g["out"])
        assert err == (g["err_v"] if verbose else g["err"])
    assert g["out"] == g["out_v"]
    plain = "".join(l + "\n" for l in g["err_v"].split("\n")[:-1]
                    if not re.match(r"(ALIGN|LINK|TEST|     tig|Processing|  Failed|$)", l))
    assert plain == g["err"]


def test_fixtures_are_small_and_reach_the_branches(runs):
    for name in GR.FIXTURES:
        assert os.path.getsize(os.path.join(GOLDEN, f"gfa_{name}.npz")) < 64 * 1024
    total = {k: 0 for k in GR.REQUIRED_BRANCHES}
    for name in GR.FIXTURES:
        log = runs[name][True][3]
        for k in GR.REQUIRED_BRANCHES:
            total[k] += log[k]
    assert [k for k in GR.REQUIRED_BRANCHES if total[k] == 0] == []
    # both outcomes in one fixture of every mode
    a, b, d = (runs[n][True][3] for n in "abd")
    assert a["link_kept"] and a["link_dropped"]
    assert b["rec_kept"] and b["rec_dropped"]
    assert d["link_kept"] and d["link_star"]
    assert max(runs[n][True][3]["rounds_max"] for n in GR.FIXTURES) >= 5


def test_fixture_lengths_are_ungapped():
    """The LN:i: values the reference printed are the lengths the encoder's stores decode to."""
    g = GR.golden("a")
    T = GR.store_tigs(g["gapped_T"])
    assert any(b"-" in (t or b"") for t in g["gapped_T"])
    for m in re.finditer(r"S\ttig(\d+)\t\*\tLN:i:(\d+)\n", g["out"]):
        assert len(T[int(m.group(1))]) == int(m.group(2))
    assert T[8] == b"" and g["gapped_T"][8] is None


@pytest.mark.skipif(not os.path.exists(REF_OBJ), reason="the reference's objects are not built")
def test_reference_on_fresh_jobs(tmp_path):
    """Three fresh random jobs per mode through the reference, rebuilt here, and the
    restatement."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_gfa_golden as MG
    bd = str(tmp_path / "ref")
    os.makedirs(bd)
    ref = MG.build_reference(bd)
    for seed in (1, 2, 3):
        job = G.synth_graph(seed=seed, n_links=10, n_records=6, tig_len=2500, overlap=500,
                            error_rate=0.03, false_every=4, ctg_len=9000, utg_len=1500)
        bed_gfa = "".join("ctg%08d\t%d\t%d\tutg%08d\t0\t+\n" % (k // 4, 120 * (k % 4),
                                                              120 * (k % 4) + 2500, k) for k in range(8))
        for args, C, text in (("-T T.tigStore 2 -gfa -i in -o out", None, job["gfa_text"]),
                              ("-T T.tigStore 2 -C C.tigStore 2 -bed -i in -o out", job["ctgs"],
                               job["bed_text"]),
                              ("-T T.tigStore 2 -bed -i in -o out", None, bed_gfa)):
            for verbose in (False, True):
                want_out, want_err, _ = MG.run_reference(ref, args.split(), job["utgs"], C, text, verbose)
                out, err, _ = GR.run(args.split() + (["-V"] if verbose else []), job["utgs"], C, text)
                assert out == want_out and err == want_err, (seed, args, verbose)


# ------------------------------------------------------------------ the text helpers

def _link_results(res):
    """The restatement's per-link results as check_links returns them."""
    out = np.zeros(len(res), dtype=G.LINK_RESULT_DTYPE)
    runs = []
    for i, r in enumerate(res):
        for f in ("max_edit", "a_len", "b_len", "abgn_b", "bend_b", "dist_b", "bend", "abgn_a",
                  "dist_a", "abgn", "dist_f", "align_len"):
            out[i][f] = r[f]
        out[i]["success"] = r["success"]
        mine = GR.cigar_runs(r["cigar"]) if r["success"] else []
        out[i]["run_off"], out[i]["n_runs"] = len(runs), len(mine)
        runs += [(n, ord(op)) for n, op in mine]
    return out, np.array(runs, dtype=G.RUN_DTYPE).reshape(-1)


def _record_results(res):
    out = np.zeros(len(res), dtype=G.RECORD_RESULT_DTYPE)
    tries = []
    for i, (ok, bgn, end, tr) in enumerate(res):
        out[i] = (ok, bgn, end, len(tr), len(tries))
        tries += [(i, t["call"], t["b_len"], t["abgn"], t["aend"], t["max_edit"], t["dist"],
                   t["nbgn"], t["nend"], t["outcome"]) for t in tr]
    return out, np.array(tries, dtype=G.TRY_DTYPE).reshape(-1)


@pytest.mark.parametrize("name", GR.FIXTURES)
def test_text_helpers_equal_the_restatement(runs, name):
    """canu_amd.align_gfa's parsers and writers, fed the restatement's results, give its text."""
    g = GR.golden(name)
    T = GR.store_tigs(g["gapped_T"])
    lens_T = [len(t) for t in T]
    for verbose, (out, err, res, _) in runs[name].items():
        o = G.parse_alignGFA_args(g["args"] + (["-V"] if verbose else []))
        assert o == GR.parse_args(g["args"] + (["-V"] if verbose else []))
        if o["type"] == "gfa":
            gfa = G.parse_gfa(g["input"])
            r, rn = _link_results(res)
            got = G.gfa_output(gfa, lens_T, r, rn, o, verbose)
        elif o["C"] is not None:
            bed = G.parse_bed(g["input"])
            r, tr = _record_results(res)
            C = GR.store_tigs(g["gapped_C"])
            got = G.bed_output(bed, [len(t) for t in C], r, tr, o, verbose)
        else:
            bed = G.parse_bed(g["input"])
            links, arr, used = G.bed_links(bed)
            r, rn = _link_results(res)
            assert [(int(a["a_align"]),) for a in arr] == \
                [(p[2],) for p in GR.bed_pairs(GR.parse_bed(g["input"]))]
            got = G.bed_gfa_output(bed, links, arr, used, lens_T, r, rn, o, verbose)
        assert got == (out, err)


def test_cigar_lengths():
    for cg, want in (("500M", (500, 500, 500)), ("450M20I30M10D20M", (520, 510, 530)),
                     ("*", (0, 0, 0)), ("10=5X3N2S", (15, 18, 15)), ("300M300I", (600, 300, 600))):
        q, r, a, warn = G.cigar_lengths(cg)
        err = []
        assert (q, r, a) == want == GR.alignment_length(cg, err)
        assert warn == err
    assert G.name_to_id("tig00000012") == 12 == GR.name_to_id("ctg12")
    assert G.name_to_id("read5") == 0xFFFFFFFF == GR.name_to_id("x")


def test_synth_graph():
    job = G.synth_graph(seed=3, n_links=16, n_records=8, tig_len=1500, overlap=300, ctg_len=6000,
                        utg_len=900)
    again = G.synth_graph(seed=3, n_links=16, n_records=8, tig_len=1500, overlap=300, ctg_len=6000,
                          utg_len=900)
    assert job["gfa_text"] == again["gfa_text"] and job["utgs"] == again["utgs"]
    assert len(job["utgs"]) == 17 + 8 and job["links"].shape == (16,) and job["records"].shape == (8,)
    assert {(int(l["a_fwd"]), int(l["b_fwd"])) for l in job["links"]} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    gfa = G.parse_gfa(job["gfa_text"])
    assert np.array_equal(gfa["array"], job["links"])
    assert np.array_equal(G.parse_bed(job["bed_text"])["array"], job["records"])
    # true links align, false ones do not
    log = GR.new_log()
    _, _, res = GR.process_gfa(job["utgs"], job["gfa_text"], {"in": "i", "out": "o", "T": "t", "Tv": 2},
                               False, log)
    assert [r["success"] for r in res] == [i % 8 != 7 for i in range(16)]


# ------------------------------------------------------------------ refusals

def test_refusals():
    tigs = [b"ACGT" * 100, b"ACGT" * 100, b""]
    log = GR.new_log()

    def link(a, b, cigar):
        return {"Aid": a, "Afwd": True, "Bid": b, "Bfwd": True, "cigar": cigar, "Aname": "a",
                "Bname": "b"}
    for bad in (link(3, 1, "100M"), link(0, 0xFFFFFFFF, "100M"), link(2, 1, "100M"),
                link(0, 2, "100M"), link(0, 1, "*"), link(0, 1, "100I"), link(0, 1, "100D")):
        with pytest.raises(GR.Refused):
            GR.check_link(bad, tigs, log, None)
    assert GR.check_link(link(0, 1, "100M"), tigs, log, None)["success"]

    def rec(a, b, bgn, end):
        return {"Aid": a, "Bid": b, "Bfwd": True, "bgn": bgn, "end": end, "Aname": "c",
                "Bname": "u", "score": 0}
    for bad in (rec(3, 0, 0, 100), rec(0, 3, 0, 100), rec(2, 0, 0, 0), rec(0, 2, 0, 100),
                rec(0, 1, -1, 100), rec(0, 1, 0, 401), rec(0, 1, 200, 100)):
        with pytest.raises(GR.Refused):
            GR.check_record(bad, tigs, tigs, log, None)
    for text in ("S\ttig1\t*\n", "L\ttig1\t+\ttig2\t+\n", "X\tfoo\n", "Hx\n"):
        with pytest.raises(GR.Refused):
            GR.parse_gfa(text)
        with pytest.raises(ValueError):
            G.parse_gfa(text)
    with pytest.raises(GR.Refused):
        GR.parse_bed("ctg1\t0\t10\tutg1\t0\n")
    with pytest.raises(ValueError):
        G.parse_bed("ctg1\t0\t10\tutg1\t0\n")
    # a name that is not tig, utg or ctg and a number is a tig outside every store
    assert GR.parse_gfa("L\tread1\t+\ttig2\t+\t5M\n")[2][0]["Aid"] == 0xFFFFFFFF
    for argv in (["-G", "g", "-T", "t", "2", "-i", "i", "-o", "o"], ["-T", "t", "2", "-i", "i"],
                 ["-T", "t", "0", "-i", "i", "-o", "o"], ["-i", "i", "-o", "o"],
                 ["-T", "t", "2", "-C", "c", "0", "-i", "i", "-o", "o"]):
        with pytest.raises(ValueError):
            G.parse_alignGFA_args(argv)
        with pytest.raises(ValueError):
            GR.parse_args(argv)


# ------------------------------------------------------------------ the ABI

def _header():
    return open(os.path.join(ROOT, "include", "canu_gfa.h")).read()


def test_header_and_binding_agree():
    h = _header()
    assert int(re.search(r"#define GFA_ABI_VERSION (\d+)", h).group(1)) == G.ABI_VERSION
    assert int(re.search(r"#define GFA_END_BASES (\d+)", h).group(1)) == G.END_BASES == GR.END_BASES
    assert int(re.search(r"#define GFA_LEAF_BYTES (\d+)", h).group(1)) == G.LEAF_BYTES == GR.FS.LEAF_BYTES
    for name, code in re.findall(r"(GFA_(?:OK|ERR_\w+)) = (-?\d+)", h):
        assert G.GFA_STATUS[int(code)] == name
    declared = re.findall(r"\b(gfa_\w+)\s*\(", h.split("typedef struct gfa_ctx gfa_ctx;")[1])
    assert sorted(set(declared)) == sorted(G.EXPORTS)


def test_structure_sizes(tmp_path):
    """The binding's dtypes have the sizes and offsets the C compiler gives the header's
    structures."""
    cc = shutil.which(os.environ.get("CC", "gcc")) or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    structs = {"gfa_link": G.LINK_DTYPE, "gfa_link_result": G.LINK_RESULT_DTYPE, "gfa_run": G.RUN_DTYPE,
               "gfa_record": G.RECORD_DTYPE, "gfa_record_result": G.RECORD_RESULT_DTYPE,
               "gfa_try": G.TRY_DTYPE}
    src = ['#include <stddef.h>\n#include <stdio.h>\n#include "canu_gfa.h"\nint main(void) {\n']
    for s, dt in structs.items():
        src.append(f'  printf("{s} %zu", sizeof({s}));\n')
        for f in dt.names:
            src.append(f'  printf(" %zu", offsetof({s}, {f}));\n')
        src.append('  printf("\\n");\n')
    src.append('  printf("gfa_params %zu\\n", sizeof(gfa_params));\n')
    src.append('  printf("gfa_stats %zu\\n", sizeof(gfa_stats));\n  return 0;\n}\n')
    c = tmp_path / "sizes.c"
    c.write_text("".join(src))
    exe = str(tmp_path / "sizes")
    subprocess.run([cc, "-I" + os.path.join(ROOT, "include"), "-o", exe, str(c)], check=True)
    lines = dict(l.split(" ", 1) for l in subprocess.run([exe], capture_output=True, text=True,
                                                          check=True).stdout.strip().split("\n"))
    for s, dt in structs.items():
        want = [dt.itemsize] + [dt.fields[f][1] for f in dt.names]
        assert [int(x) for x in lines[s].split()] == want, s
    assert int(lines["gfa_params"]) == ctypes.sizeof(G._Params)
    assert int(lines["gfa_stats"]) == ctypes.sizeof(G._Stats)


# ------------------------------------------------------------------ the host code, sanitized

def _write_store(path, gapped):
    os.makedirs(path)
    tig, dat = GR.encode_tigstore(gapped)
    for ext, raw in (("tig", tig), ("dat", dat)):
        with open(os.path.join(path, "seqDB.v002." + ext), "wb") as f:
            f.write(raw)


def _arith_cases(g, T, C):
    """gfa_host.h's arithmetic against the numbers the reference's -V log holds."""
    cases = []
    v = g["err_v"]
    link = re.compile(
        r"LINK tig(\d+) . +tig(\d+) . +Aalign +(\d+) Balign +(\d+) align +(\d+)\n"
        r"TEST tig\d+ . +(\d+)-(\d+) +tig\d+ . +\d+-(\d+) +maxEdit= *(\d+)  \(extend B\).*\n"
        r"     tig\d+ . +(\d+)-\d+ +tig\d+ . +\d+-\d+ +maxEdit= *\d+  \(extend A\)")
    for m in link.finditer(v):
        a, b, aa, ba, al, abgn_b, alen, bend_b, me, abgn_a = (int(x) for x in m.groups())
        assert alen == len(T[a])
        cases.append(f"link {alen} {len(T[b])} {aa} {ba} {al} {me} {abgn_b} {bend_b} {abgn_a}")
    align = re.compile(r"ALIGN +(\w+) utg \S+ len= *(\d+) to ctg \S+ +(\d+)- *(\d+) len= *(\d+)"
                       r"( - POSITION from +\d+-\d+ +to +(\d+)-(\d+) +score +(\d+)/ *(\d+) = +(-?\d+)| - FAILED, RELAX)?")
    for m in align.finditer(v):
        blen = int(m.group(2))
        if m.group(7) is not None:
            nb, ne, d, al, sc = (int(m.group(i)) for i in (7, 8, 9, 10, 11))
            cases.append(f"score {nb} {ne} {blen} {d} {al} {sc}")
    if C is not None:
        # the first try of the first record: its window and maxEdit from the record alone
        r = GR.parse_bed(g["input"])[0]
        m = next(align.finditer(v))
        blen = int(m.group(2))
        bgn, end = r["bgn"], r["end"]
        if m.group(1) == "LEFT":
            end = bgn + GR.END_BASES
        me = int(np.ceil(blen * 0.03))
        cases.append(f"window {m.group(5)} {blen} {bgn} {end} {int(m.group(3))} {int(m.group(4))} {me}")
    return cases


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("gfa_host")
    exe = str(d / "gfa_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wall", "-o", exe,
                    os.path.join(ROOT, "tests", "gfa_host_check.cpp")], check=True)
    return exe


def test_host_code_under_sanitizers(host_check, tmp_path):
    d = str(tmp_path)
    cases = []
    for name in GR.FIXTURES:
        g = GR.golden(name)
        kind = "gfa" if "-gfa" in g["args"] else "bed"
        with open(os.path.join(d, f"{name}.in"), "w") as f:
            f.write(g["input"])
        cases.append(f"{kind} {name}.in")
        if g["out"].startswith("H\t"):                 # the output files parse and write too
            with open(os.path.join(d, f"{name}.out"), "w") as f:
                f.write(g["out"])
            if "\t*\n" not in g["out"].replace("\t*\tLN", ""):
                cases.append(f"gfa {name}.out")
        T = C = None
        for which in ("T", "C"):
            gapped = g["gapped_" + which]
            if gapped is None:
                continue
            _write_store(os.path.join(d, f"{name}.{which}"), gapped)
            seqs = GR.store_tigs(gapped)
            with open(os.path.join(d, f"{name}.{which}.want"), "wb") as f:
                f.write(b"".join(s + b"\n" for s in seqs))
            cases.append(f"store {name}.{which} 2 {name}.{which}.want")
            cases.append(f"store {name}.{which} 7 {name}.{which}.want")     # the nearest version below
            if name in ("a", "b", "d"):
                cases.append(f"damage {name}.{which} 2")
            T, C = (seqs, C) if which == "T" else (T, seqs)
        cases += _arith_cases(g, T, C)
    bad = {"bad1.gfa": "S\ttig1\t*\n", "bad2.gfa": "L\ttig1\t+\ttig2\t+\n", "bad3.gfa": "L\ttig1\n",
           "bad4.gfa": "Q\tx\n", "bad5.gfa": "S tig1 * LN:i:4\n", "bad1.bed": "ctg1\t0\t10\tutg1\t0\n",
           "bad2.bed": "ctg1\n"}
    for fn, text in bad.items():
        with open(os.path.join(d, fn), "w") as f:
            f.write(text)
        cases.append(("badgfa " if fn.endswith("gfa") else "badbed ") + fn)
    cases += ["cigar 500M 500 500 500", "cigar 450M20I30M10D20M 520 510 530", "cigar * 0 0 0",
              "cigar 10=5X3N2S 15 18 15", "cigar 7 0 0 0", "cigar M 0 0 0",
              "relax 15 18", "relax 24 28", "relax 1500 1800", "relax 4 4",
              "ratio 0 500 0.0000", "ratio 31 1033 0.0300", "link 400 3000 500 500 500 60 0 550 0"]
    me = 15
    for _ in range(12):                                # maxEdit *= 1.2 along a RELAX chain
        nxt = int(me * 1.2)
        cases.append(f"relax {me} {nxt}")
        me = nxt
    with open(os.path.join(d, "cases.txt"), "w") as f:
        f.write("\n".join(cases) + "\n")
    assert sum(c.startswith("link ") for c in cases) >= 15
    assert sum(c.startswith("score ") for c in cases) >= 8
    cp = subprocess.run([host_check, d], capture_output=True, text=True)
    assert cp.returncode == 0, cp.stdout[-3000:] + cp.stderr[-3000:]
    assert f"{len(cases)} cases, 0 failures" in cp.stdout
