"""falconsense on the GPU (libcanu_fs.so and canu_amd/bin/falconsense): the reference's stdout
and stderr on the fixtures, and lengths, leaf / split shapes, windows, coverage and piece
boundaries, batches and error returns against the Python restatement (tests/fs_restate.py,
itself pinned to the reference by tests/test_fs_cpu.py)."""
import os
import subprocess

import numpy as np
import pytest

import fs_restate as FS
from canu_amd import falconsense as F
from canu_amd.synth import ReadSet

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _rand(rng, n):
    return _ACGT[rng.integers(0, 4, n)].tobytes()


def _rc(b):
    return b.translate(bytes.maketrans(b"ACGTN", b"TGCAN"))[::-1]


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


def _arrays(tigs):
    """tigs: [(tig_id, [(ident, reverse, min, max, askip, bskip), ...])]"""
    lay, kids = [], []
    for tid, ch in tigs:
        lay.append((tid, len(kids), len(ch)))
        kids += ch
    return (np.array(lay, dtype=F.LAYOUT_DTYPE).reshape(-1),
            np.array(kids, dtype=F.CHILD_DTYPE).reshape(-1))


def _check(reads, tigs, params=None):
    """The library against the restatement: consensus, counters, leaves and splits, cells."""
    params = params or F.FsParameters()
    lay, kids = _arrays(tigs)
    fs = F.FalconSense(params)
    fs.load_reads(_read_set(reads))
    got = fs.run(lay, kids)
    cnt, st, fasta = fs.counters().copy(), fs.stats(), fs.fasta_bytes()
    fs.close()
    rd = {i + 1: r for i, r in enumerate(reads)}
    log = FS.new_log()
    want_fasta = bytearray()
    for k, (tid, ch) in enumerate(tigs):
        want, wc = FS.correct_tig(rd, tid, ch, params.min_coverage, params.min_identity, log,
                                  integer=True)
        assert got[k] == want, (tid, len(got[k]), len(want))
        assert cnt[k].tolist() == wc, (tid, cnt[k].tolist(), wc)
        for j, p in enumerate(FS.pieces(want, params.min_output_length)):
            want_fasta += FS.fasta_record(tid, j, p)
    assert fasta == bytes(want_fasta)
    assert (st["n_leaves"], st["n_splits"]) == (log["leaf"], log["split"])
    assert st["dp_cells"] == log["cells"]
    return got, st, log


def _child(rng, tmpl, s, e, err=0.05, reverse=False, ident=None):
    seq = _mutate(rng, tmpl[s:e], err)
    return (_rc(seq) if reverse else seq), (ident, int(reverse), s, e, 0, 0)


def _tig(rng, tlen, spans, err=0.05):
    """One template of tlen bases (read 1) and a child per span -> (reads, tigs)."""
    tmpl = _rand(rng, tlen)
    reads, ch = [tmpl], []
    for k, (s, e) in enumerate(spans):
        seq, c = _child(rng, tmpl, s, e, err, reverse=bool(k & 1))
        reads.append(seq)
        ch.append((len(reads),) + c[1:])
    return reads, [(1, ch)]


def _selected_layouts(g):
    o = FS.parse_args(g["args"])
    sel = FS.selected(o, len(g["lengths"]), g["read_list"])
    return o, g["layouts"][np.isin(g["layouts"]["tig_id"], sel)]


@pytest.mark.parametrize("name", FS.FIXTURES)
def test_fixture_equals_reference(built, name):
    g = FS.golden(name)
    o, lay = _selected_layouts(g)
    fs = F.FalconSense(F.FsParameters(o["cc"], o["ci"], o["cl"]))
    fs.load_reads(ReadSet(bases=g["bases"], offsets=g["offsets"], lengths=g["lengths"], first_iid=1))
    fs.run(lay, g["children"])
    assert fs.fasta_bytes() == g["stdout"]
    cnt = fs.counters()
    assert tuple(int(v) for v in cnt.sum(axis=0)) == FS.EXPECTED_COUNTS[name]
    assert np.array_equal(cnt.sum(axis=1), lay["n_children"] + 1)
    fs.close()


def test_write_fasta_equals_fasta_bytes(built, tmp_path):
    g = FS.golden("f")
    o, lay = _selected_layouts(g)
    fs = F.FalconSense(F.FsParameters(o["cc"], o["ci"], o["cl"]))
    fs.load_reads(ReadSet(bases=g["bases"], offsets=g["offsets"], lengths=g["lengths"], first_iid=1))
    fs.run(lay, g["children"])
    fs.write_fasta(str(tmp_path / "out.fasta"))
    assert (tmp_path / "out.fasta").read_bytes() == g["stdout"] == fs.fasta_bytes()
    fs.close()


@pytest.mark.parametrize("name", FS.FIXTURES)
def test_executable_equals_reference(built, name, tmp_path):
    import oracle
    g = FS.golden(name)
    gkp = oracle.build_gkpstore(ReadSet(bases=g["bases"], offsets=g["offsets"],
                                        lengths=g["lengths"], first_iid=1), str(tmp_path))
    cor = tmp_path / "asm.corStore"
    cor.mkdir()
    (cor / "seqDB.v001.tig").write_bytes(g["tig"])
    (cor / "seqDB.v001.dat").write_bytes(g["dat"])
    cmd = [os.path.join(ROOT, "canu_amd", "bin", "falconsense"), "-G", gkp, "-C", str(cor), "-t", "4",
           "-p", str(tmp_path / "asm"), *g["args"]]
    if g["read_list"] is not None:
        (tmp_path / "readlist").write_text("".join(f"{i}\n" for i in g["read_list"]))
        cmd += ["-r", str(tmp_path / "readlist")]
    cp = subprocess.run(cmd, capture_output=True)
    assert cp.returncode == 0, cp.stderr[-2000:]
    assert cp.stdout == g["stdout"]
    assert cp.stderr == g["stderr"]


def test_executable_refuses_a_cut_store(built, tmp_path):
    import oracle
    g = FS.golden("e")
    gkp = oracle.build_gkpstore(ReadSet(bases=g["bases"], offsets=g["offsets"],
                                        lengths=g["lengths"], first_iid=1), str(tmp_path))
    cor = tmp_path / "asm.corStore"
    cor.mkdir()
    (cor / "seqDB.v001.tig").write_bytes(g["tig"])
    (cor / "seqDB.v001.dat").write_bytes(g["dat"][:len(g["dat"]) - 10])
    cp = subprocess.run([os.path.join(ROOT, "canu_amd", "bin", "falconsense"), "-G", gkp, "-C",
                         str(cor), *g["args"]], capture_output=True)
    assert cp.returncode == 1 and b"data file" in cp.stderr and cp.stdout == b""


def test_evidence_lengths(built):
    """499 is skipped, 500 is not; 511 / 512 / 513 cross a 64-row block, 4,097 a lane stripe."""
    rng = np.random.default_rng(41)
    lens = [499, 500, 511, 512, 513, 4097]
    tmpl = _rand(rng, 4400)
    reads, ch = [tmpl], []
    for k, L in enumerate(lens):
        s = 0 if L > 4000 else 300 + 97 * k
        seq = _mutate(rng, tmpl[s:s + L + 40], 0.06)[:L]
        assert len(seq) == L
        reads.append(_rc(seq) if k & 1 else seq)
        ch.append((len(reads), k & 1, s, s + L, 0, 0))
    got, st, log = _check(reads, [(1, ch)])
    assert (log["skipped"], log["aligned"]) == (1, 6)


@pytest.mark.parametrize("tlen,leaf", [(1790, True), (1800, False)])
def test_leaf_rule_at_the_top(built, tlen, leaf):
    """q = t = 1,790 is a leaf (28 blocks: 568 x 1,790 < 1,048,576), q = t = 1,800 a split (29
    blocks: 588 x 1,800): the template against itself is exactly that pair."""
    assert FS.is_leaf(tlen, tlen) == leaf
    rng = np.random.default_rng(tlen)
    reads, tigs = _tig(rng, tlen, [])
    got, st, log = _check(reads, tigs)
    assert (st["n_leaves"], st["n_splits"]) == ((1, 0) if leaf else (2, 1))
    copies = [reads[0]] + [reads[0]] * 5                 # and with five exact copies as evidence
    _check(copies, [(1, [(k, 0, 0, tlen, 0, 0) for k in range(2, 7)])])


def test_leaf_rule_below_the_top(built):
    """A top-level target is at most twice its query (the distance is at most the query), so
    q = 1,000 against t = 3,196 / 3,197 (16 blocks: 328 x t crosses 1,048,576) can only be a
    half of a larger problem.  Evidence with one deletion of 2,300 bases gives halves much wider
    than they are tall; the leaves and splits the device counts equal the restatement's."""
    assert FS.is_leaf(1000, 3196) and not FS.is_leaf(1000, 3197)
    rng = np.random.default_rng(43)
    tmpl = _rand(rng, 7900)
    for cut in (2500, 2963, 3301):
        ev = _mutate(rng, tmpl[100:cut], 0.03) + _mutate(rng, tmpl[cut + 2300:7800], 0.03)
        got, st, log = _check([tmpl, ev], [(1, [(2, 0, 100, 7800, 0, 0)])])
        assert log["aligned"] == 2 and log["max_depth"] >= 2


def test_indel_runs_at_both_ends(built):
    """Evidence whose ends do not belong to the template: the alignment starts and ends with
    runs of insertions, which are stripped, and deletions."""
    rng = np.random.default_rng(44)
    tmpl = _rand(rng, 2400)
    reads, ch = [tmpl], []
    for k, (s, e) in enumerate([(300, 1500), (600, 2100), (900, 2000)]):
        core = _mutate(rng, tmpl[s:e], 0.04)
        seq = b"T" * (5 + 3 * k) + core[:200] + core[230:-220] + core[-200:] + b"G" * (4 + k)
        reads.append(seq)
        ch.append((len(reads), 0, s, e, 0, 0))
    _check(reads, [(1, ch)])


def test_windows(built):
    """The window is clamped at both template ends; an expansion <= 0 leaves it as placed."""
    rng = np.random.default_rng(45)
    tmpl = _rand(rng, 2600)
    reads, ch, exps = [tmpl], [], []
    for (s, e, mn, mx) in [(0, 900, 0, 900), (1700, 2600, 1700, 2600), (0, 2600, 0, 2600),
                           (800, 1700, 600, 2000), (900, 1600, 500, 2100), (10, 800, 0, 700)]:
        reads.append(_mutate(rng, tmpl[s:e], 0.05))
        ch.append((len(reads), 0, mn, mx, 0, 0))
        exps.append(int((1.4 * len(reads[-1]) - (mx - mn)) / 2))
    assert [x <= 0 for x in exps] == [False, False, False, True, True, False]
    _check(reads, [(1, ch)])


def test_skips_and_orientation(built):
    rng = np.random.default_rng(46)
    tmpl = _rand(rng, 2500)
    reads, ch = [tmpl], []
    for k, (s, e, a, b) in enumerate([(200, 1800, 150, 90), (500, 2400, 0, 310), (100, 1500, 77, 0)]):
        core = _mutate(rng, tmpl[s:e], 0.05)
        rev = k != 1
        seq = _rand(rng, a) + core + _rand(rng, b)        # the oriented read: skips, then reversed
        reads.append(_rc(seq) if rev else seq)
        ch.append((len(reads), int(rev), s, e, a, b))
    _check(reads, [(1, ch)])


def test_no_children_and_short_template(built):
    rng = np.random.default_rng(47)
    reads = [_rand(rng, 1300), _rand(rng, 480), _rand(rng, 900)]
    got, st, log = _check(reads, [(1, []), (2, []), (2, [(3, 0, 0, 480, 0, 0)])])
    assert len(got[0]) == 1299 and got[0] == got[0].lower()     # itself, less the first column
    assert got[1] == b"" and got[2] == b""                       # where the reference asserts


def test_minimum_coverage_boundary(built):
    """-cc 4: coverage 4 (the template and three children) is lower case, coverage 5 is not."""
    rng = np.random.default_rng(48)
    tmpl = _rand(rng, 1500)
    reads = [tmpl] + [_mutate(rng, tmpl, 0.02) for _ in range(4)]
    kids = [(k, 0, 0, 1500, 0, 0) for k in range(2, 6)]
    got, _, _ = _check(reads, [(1, kids[:3]), (1, kids)], F.FsParameters(min_coverage=4))
    assert got[0] == got[0].lower() and got[0]
    assert sum(c < 97 for c in got[1]) > 1400


def test_piece_length_boundary(built):
    """-cl 500: a piece of 500 bases is not written, one of 501 is."""
    rng = np.random.default_rng(49)
    tmpl = _rand(rng, 1600)
    out = []
    for span in (500, 501):
        reads = [tmpl] + [tmpl[400:400 + span]] * 5
        kids = [(k, 0, 400, 400 + span, 0, 0) for k in range(2, 7)]
        got, _, _ = _check(reads, [(1, kids)], F.FsParameters(min_output_length=500))
        out.append([len(p) for p in FS.pieces(got[0], 0) if len(p) >= 400])
    assert out == [[500], [501]]
    assert len(FS.pieces(b"A" * 500, 500)) == 0 and len(FS.pieces(b"A" * 501, 500)) == 1


def test_batches_by_budget(built):
    """A budget smaller than one layout runs every layout as a batch of its own; the results do
    not change.  (Every device buffer has an exact upper bound -- an alignment of q rows over a
    window of w columns has at most q + w tags -- so nothing can overflow and there is no
    launch to repeat with grown buffers.)"""
    g = FS.golden("e")
    o, lay = _selected_layouts(g)
    rs = ReadSet(bases=g["bases"], offsets=g["offsets"], lengths=g["lengths"], first_iid=1)
    outs = []
    for budget in (0, 1 << 20):
        fs = F.FalconSense(F.FsParameters(o["cc"], o["ci"], o["cl"], hbm_budget=budget))
        fs.load_reads(rs)
        fs.run(lay, g["children"])
        outs.append((fs.fasta_bytes(), fs.counters().tolist(), fs.stats()["n_batches"]))
        fs.close()
    assert outs[0][:2] == outs[1][:2] and outs[0][0] == g["stdout"]
    assert (outs[0][2], outs[1][2]) == (1, len(lay))


def test_min_identity(built):
    """min_identity 0.7 as a double: pinned to the restatement only, since the reference program
    cannot be given a fraction.  A child at 45 % error is rejected by the tolerance, one at 25 %
    passes it."""
    rng = np.random.default_rng(50)
    tmpl = _rand(rng, 2300)
    reads, ch = [tmpl], []
    for err in (0.03, 0.10, 0.25, 0.45, 0.60):
        reads.append(_mutate(rng, tmpl[200:2000], err))
        ch.append((len(reads), 0, 200, 2000, 0, 0))
    reads.append(_rand(rng, 1200))                               # no relation at all
    ch.append((len(reads), 0, 500, 1700, 0, 0))
    got, st, log = _check(reads, [(1, ch)], F.FsParameters(min_identity=0.7))
    assert log["rejected"] >= 2 and log["aligned"] >= 3


def test_error_returns(built):
    rng = np.random.default_rng(51)
    reads = [_rand(rng, 900), _rand(rng, 800)]
    fs = F.FalconSense()
    fs.load_reads(_read_set(reads))

    def code(tigs):
        lay, kids = _arrays(tigs)
        with pytest.raises(F.FsError) as e:
            fs.run(lay, kids)
        return e.value.code

    assert code([(3, [])]) == -4                                  # a template that is not loaded
    assert code([(1, [(7, 0, 0, 800, 0, 0)])]) == -4              # a child that is not loaded
    assert code([(1, [(2, 0, 0, 800, 500, 301)])]) == -4          # skips longer than the read
    assert code([(1, [(2, 0, 0, 800, -1, 0)])]) == -4
    assert code([(1, [(2, 0, 400, 400, 0, 0)])]) == -4            # max <= min
    assert code([(1, [(2, 0, 0, 800, 0, 0)] * 65536)]) == -4      # more than 65,535 children
    lay, kids = _arrays([(1, [(2, 0, 0, 800, 0, 0)])])
    lay["n_children"] = 2
    with pytest.raises(F.FsError) as e:
        fs.run(lay, kids)
    assert e.value.code == -2                                     # children past the array
    with pytest.raises(F.FsError) as e:
        fs.load_reads(_read_set([b"ACGTXACGT"]))
    assert e.value.code == -4
    fs.close()
    with pytest.raises(F.FsError):
        F.FalconSense(F.FsParameters(min_identity=1.5))


def test_abi_symbols(built):
    import ctypes
    lib = ctypes.CDLL(F.LIB_PATH)
    for s in F.EXPORTS:
        assert hasattr(lib, s), s
    assert lib.fs_abi_version() == F.ABI_VERSION
