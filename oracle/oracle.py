"""Python access to the parity checkers (TEST INFRASTRUCTURE ONLY).

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg import this module.
  * run_oracle(...)    -- the C restatement in oic_oracle.c (oracle/_build/liboic_oracle.so)
  * run_reference(...) -- the reference overlapInCore built from its own sources
                          (oracle/_ref/oic_ref, see ref_harness.cpp)
Both return records as a numpy structured array with fields a, b, w0, w1 (the ovOverlap
a_iid, b_iid and dat[0], dat[1]), sorted by ovOverlap::operator<.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "_build", "liboic_oracle.so")
REF_BIN = os.path.join(HERE, "_ref", "oic_ref")

RECORD_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("w0", "<u8"), ("w1", "<u8")])


class OracleParams(ctypes.Structure):
    _fields_ = [("kmer_len", ctypes.c_uint32), ("max_erate", ctypes.c_double),
                ("min_olap_len", ctypes.c_int32), ("partial", ctypes.c_int32),
                ("unique_olap_per_pair", ctypes.c_int32), ("use_window_filter", ctypes.c_int32),
                ("use_hopeless_check", ctypes.c_int32), ("frag_olap_limit", ctypes.c_uint64),
                ("filter_by_kmer_count", ctypes.c_uint64)]


class OracleStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in (
        "kmer_hits_without_olap", "kmer_hits_with_olap", "kmer_hits_skipped", "multi_overlaps",
        "total_overlaps", "contained_overlaps", "dovetail_overlaps", "seed_hits", "pairs")]


_lib = None


def build() -> None:
    subprocess.run(["make", "-s", "-C", HERE], check=True)


def _load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            build()
        lib = ctypes.CDLL(LIB_PATH)
        lib.oic_oracle_run.restype = ctypes.c_int
        lib.oic_oracle_run.argtypes = [
            ctypes.POINTER(OracleParams), ctypes.c_uint32, ctypes.c_uint32,
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
            ctypes.c_char_p, ctypes.c_uint64,
            ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
            ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64),
            ctypes.POINTER(OracleStats)]
        lib.oic_oracle_free.argtypes = [ctypes.c_void_p]
        lib.oic_oracle_seed_hits.restype = ctypes.c_int
        lib.oic_oracle_seed_hits.argtypes = [
            ctypes.POINTER(OracleParams), ctypes.c_uint32, ctypes.c_uint32,
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint64,
            ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
            ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64)]
        lib.oic_oracle_match_limit.restype = ctypes.c_int
        lib.oic_oracle_match_limit.argtypes = [ctypes.c_double, ctypes.c_void_p, ctypes.c_int32]
        _lib = lib
    return _lib


def default_params(**kw) -> dict:
    """oicParameters::initialize() defaults (overlapInCore.H:425), plus main()'s
    fix-up for maxErate > 0.06 (overlapInCore.C:416)."""
    p = dict(kmer_len=22, max_erate=0.06, min_olap_len=0, partial=0, unique_olap_per_pair=1,
             use_window_filter=0, use_hopeless_check=1, frag_olap_limit=(1 << 64) - 1,
             filter_by_kmer_count=0)
    p.update(kw)
    # main() parses --maxerate with strtof: the value is float-rounded.
    p["max_erate"] = float(np.float32(p["max_erate"]))
    if p["max_erate"] > 0.06:
        p["use_window_filter"] = 0
        p["use_hopeless_check"] = 0
    return p


def sort_records(rec: np.ndarray) -> np.ndarray:
    return rec[np.lexsort((rec["w1"], rec["w0"], rec["b"], rec["a"]))]


def run_oracle(rs, params: dict, hash_range=None, ref_range=None, skip_kmers=None,
               with_stats=False):
    lib = _load()
    P = OracleParams(**params)
    first = rs.first_iid
    last = first + rs.nreads - 1
    hb, he = hash_range if hash_range else (first, last)
    rb, re_ = ref_range if ref_range else (first, last)
    skip = b""
    n_skip = 0
    if skip_kmers:
        skip = b"".join(k.encode() if isinstance(k, str) else k for k in skip_kmers)
        n_skip = len(skip_kmers)
    out = ctypes.c_void_p()
    n = ctypes.c_uint64()
    st = OracleStats()
    bases = np.ascontiguousarray(rs.bases)
    offs = np.ascontiguousarray(rs.offsets, dtype=np.uint64)
    lens = np.ascontiguousarray(rs.lengths, dtype=np.uint32)
    quals = None if rs.quals is None else np.ascontiguousarray(rs.quals)
    rc = lib.oic_oracle_run(ctypes.byref(P), first, rs.nreads,
                            bases.ctypes.data, offs.ctypes.data, lens.ctypes.data,
                            None if quals is None else quals.ctypes.data,
                            skip, n_skip, hb, he, rb, re_, ctypes.byref(out), ctypes.byref(n),
                            ctypes.byref(st))
    if rc != 0:
        raise RuntimeError(f"oic_oracle_run failed: {rc}")
    count = n.value
    rec = np.zeros(count, dtype=RECORD_DTYPE)
    if count:
        ctypes.memmove(rec.ctypes.data, out.value, count * RECORD_DTYPE.itemsize)
    if out.value:
        lib.oic_oracle_free(out)
    rec = sort_records(rec)
    if with_stats:
        return rec, {f: getattr(st, f) for f, _ in OracleStats._fields_}
    return rec


SEED_HIT_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("a_pos_dir", "<u4"), ("b_pos", "<u4")])


def seed_hits(rs, params: dict, hash_range=None, ref_range=None, skip_kmers=None) -> np.ndarray:
    """Every Add_Ref call of Find_Overlaps in the reference's order (query asc, FORWARD
    then REVERSE, window asc, chain order): {query, target, window | dir << 31, target pos}."""
    lib = _load()
    P = OracleParams(**params)
    first = rs.first_iid
    last = first + rs.nreads - 1
    hb, he = hash_range if hash_range else (first, last)
    rb, re_ = ref_range if ref_range else (first, last)
    skip = b"".join(k.encode() if isinstance(k, str) else k for k in (skip_kmers or []))
    out = ctypes.c_void_p()
    n = ctypes.c_uint64()
    bases = np.ascontiguousarray(rs.bases)
    offs = np.ascontiguousarray(rs.offsets, dtype=np.uint64)
    lens = np.ascontiguousarray(rs.lengths, dtype=np.uint32)
    rc = lib.oic_oracle_seed_hits(ctypes.byref(P), first, rs.nreads, bases.ctypes.data,
                                  offs.ctypes.data, lens.ctypes.data, skip,
                                  len(skip_kmers or []), hb, he, rb, re_, ctypes.byref(out),
                                  ctypes.byref(n))
    if rc != 0:
        raise RuntimeError(f"oic_oracle_seed_hits failed: {rc}")
    h = np.zeros(n.value, dtype=SEED_HIT_DTYPE)
    if n.value:
        ctypes.memmove(h.ctypes.data, out.value, n.value * SEED_HIT_DTYPE.itemsize)
    if out.value:
        lib.oic_oracle_free(out)
    return h


def match_limit(erate: float, n: int) -> tuple[int, np.ndarray]:
    lib = _load()
    out = np.zeros(n, dtype=np.int32)
    me = lib.oic_oracle_match_limit(erate, out.ctypes.data, n)
    return me, out


def reference_available() -> bool:
    return os.path.exists(REF_BIN)


def require_reference(mhap_convert: bool = False) -> None:
    """The -m gpu parity tests compare with the reference itself (oic_ref, and mhapConvert
    for the MHAP output format).  Both are built in the build container and travel to the
    GPU box with the tree, so their absence there is a broken setup: fail, never skip."""
    missing = [p for p in [REF_BIN, OVS_BIN] + ([MHAPCONVERT_BIN] if mhap_convert else [])
               if not os.path.exists(p)]
    if missing:
        raise AssertionError(f"reference checker(s) not built: {missing} "
                             "(run __graft_entry__.build() where /root/reference exists)")


def read_ovb_reference(path: str) -> np.ndarray:
    """Records of an .ovb in FILE order, read by the reference's own ovFile reader
    (oic_ref --read-ovb, ref_harness.cpp)."""
    if not reference_available():
        raise FileNotFoundError(REF_BIN)
    with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR", "/tmp")) as wd:
        out = os.path.join(wd, "rec.bin")
        cp = subprocess.run([REF_BIN, "--read-ovb", path, out], capture_output=True, text=True)
        if cp.returncode != 0:
            raise RuntimeError(f"oic_ref --read-ovb failed: {cp.stderr[-2000:]}")
        return np.fromfile(out, dtype=RECORD_DTYPE)


def build_gkpstore(rs, workdir: str) -> str:
    """A real gkpStore of rs, written by the reference's own gkStore code
    (oic_ref --gkp-only, ref_harness.cpp); returns its path (<workdir>/ref.gkpStore)."""
    from canu_amd.synth import write_reads_file  # input writer only
    if not reference_available():
        raise FileNotFoundError(REF_BIN)
    reads = os.path.join(workdir, "reads.bin")
    write_reads_file(reads, rs)
    cp = subprocess.run([REF_BIN, reads, os.path.join(workdir, "w"), "-", "--gkp-only"],
                        capture_output=True, text=True)
    if cp.returncode != 0:
        raise RuntimeError(f"oic_ref --gkp-only failed: {cp.stderr[-2000:]}")
    return os.path.join(workdir, "w", "ref.gkpStore")


OVS_BIN = os.path.join(HERE, "_ref", "ovs_ref")


def store_available() -> bool:
    return os.path.exists(OVS_BIN)


def build_store(gkp: str, store: str, ovbs) -> int:
    """The REFERENCE ovStore build (oracle/store_harness.cpp over the reference's
    ovStoreFilter / ovStoreWriter, ovStoreBuild.C:473-655) of the given .ovb files into a
    new store directory; returns the number of overlaps stored (forward + reverse copies)."""
    if not store_available():
        raise FileNotFoundError(OVS_BIN)
    cp = subprocess.run([OVS_BIN, "--build", gkp, store, *ovbs], capture_output=True, text=True)
    if cp.returncode != 0:
        raise RuntimeError(f"ovs_ref --build failed: {cp.stderr[-2000:]}")
    return int(cp.stdout.split("STORED")[1].split()[0])


def dump_store(gkp: str, store: str) -> np.ndarray:
    """Every overlap of a store, in store order, read by the reference's ovStore reader."""
    if not store_available():
        raise FileNotFoundError(OVS_BIN)
    with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR", "/tmp")) as wd:
        out = os.path.join(wd, "store.bin")
        cp = subprocess.run([OVS_BIN, "--dump", gkp, store, out], capture_output=True, text=True)
        if cp.returncode != 0:
            raise RuntimeError(f"ovs_ref --dump failed: {cp.stderr[-2000:]}")
        return np.fromfile(out, dtype=RECORD_DTYPE)


FE_BIN = os.path.join(HERE, "_ref", "fe_ref")


def fe_reference_available() -> bool:
    """The reference findErrors and what builds its two stores."""
    return os.path.exists(FE_BIN) and reference_available() and store_available()


def run_find_errors(rs, records, bgn: int, end: int, args, binary: str | None = None):
    """The REFERENCE findErrors (oracle/_ref/fe_ref, the reference's own main()) on reads rs and
    overlap records, each given once: the gkpStore by build_gkpstore, the overlap store by
    build_store, the command line canu's (OverlapErrorAdjustment.pm:194-202) with `args`
    added.  -> (.red bytes, passed, failed, the store's records of [bgn, end] in store order,
    which is what Read_Olaps loads)."""
    import re
    from canu_amd.overlap_in_core import write_ovb  # input writer only
    binary = binary or FE_BIN
    if not os.path.exists(binary):
        raise FileNotFoundError(binary)
    inp = np.asarray(records, dtype=RECORD_DTYPE)
    with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR", "/tmp")) as d:
        gkp = build_gkpstore(rs, d)
        ovb = os.path.join(d, "in.ovb")
        write_ovb(inp, ovb, counts=False)
        store = os.path.join(d, "asm.ovlStore")
        build_store(gkp, store, [ovb])
        stored = dump_store(gkp, store)
        red = os.path.join(d, "1.red")
        cp = subprocess.run([binary, "-G", gkp, "-O", store, "-R", str(bgn), str(end), *args,
                             "-l", "500", "-o", red, "-t", "4"], capture_output=True, text=True)
        if cp.returncode != 0:
            raise RuntimeError(f"findErrors failed ({cp.returncode}): {cp.stderr[-2000:]}")
        with open(red, "rb") as f:
            raw = f.read()
    passed = int(re.search(r"Passed overlaps =\s+(\d+)", cp.stderr).group(1))
    failed = int(re.search(r"Failed overlaps =\s+(\d+)", cp.stderr).group(1))
    sel = stored[(stored["a"] >= bgn) & (stored["a"] <= end)]
    return raw, passed, failed, sel


MHAPCONVERT_BIN = os.path.join(HERE, "_ref", "mhapConvert")


def mhap_convert_available() -> bool:
    return os.path.exists(MHAPCONVERT_BIN) and os.path.exists(REF_BIN)


def mhap_convert(rs, mhap_path: str, hash_base: int = 1, num_hash: int | None = None,
                 query_base: int = 1) -> np.ndarray:
    """Run the REFERENCE mhapConvert (src/mhap/mhapConvert.C, built from its source) on an
    MHAP text file against a gkpStore of rs (built by the reference's gkStore code via
    oic_ref --gkp-only); return the ovOverlap records of the .ovb it writes, in file order
    (read back with the reference's ovFile reader)."""
    from canu_amd.synth import write_reads_file  # input writer only
    if not mhap_convert_available():
        raise FileNotFoundError(MHAPCONVERT_BIN)
    nh = rs.nreads if num_hash is None else num_hash
    with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR", "/tmp")) as wd:
        reads = os.path.join(wd, "reads.bin")
        write_reads_file(reads, rs)
        cp = subprocess.run([REF_BIN, reads, os.path.join(wd, "w"), "-", "--gkp-only"],
                            capture_output=True, text=True)
        if cp.returncode != 0:
            raise RuntimeError(f"oic_ref --gkp-only failed: {cp.stderr[-2000:]}")
        ovb = os.path.join(wd, "mhap.ovb")
        cp = subprocess.run([MHAPCONVERT_BIN, "-G", os.path.join(wd, "w", "ref.gkpStore"),
                             "-o", ovb, "-h", str(hash_base), str(nh), "-q", str(query_base),
                             mhap_path], capture_output=True, text=True)
        if cp.returncode != 0:
            raise RuntimeError(f"mhapConvert failed ({cp.returncode}): {cp.stderr[-2000:]}")
        return read_ovb_reference(ovb)


def params_to_ref_args(params: dict) -> list[str]:
    a = ["-k", str(params["kmer_len"]), "--maxerate", repr(params["max_erate"]),
         "--minlength", str(params["min_olap_len"])]
    if params.get("partial"):
        a.append("-G")
    a.append("-u" if params.get("unique_olap_per_pair", 1) else "-m")
    if params.get("use_window_filter"):
        a.append("-w")
    if not params.get("use_hopeless_check", 1):
        a.append("-z")
    lim = params.get("frag_olap_limit", (1 << 64) - 1)
    if lim != (1 << 64) - 1:
        a += ["-l", str(lim)]
    return a


UINT32_MAX = 0xFFFFFFFF
ENTRIES_PER_BUCKET = 21                       # overlapInCore.H:102


def first_read_kmers(rs, bgn: int, end: int, k: int, loadable) -> np.ndarray:
    """Per read bgn..end: how many distinct k-mers of the batch first occur in it -- the
    Hash_Entries growth of Hash_Insert (Build_Hash_Index.C:336-341).  Windows holding a
    non-ACGT base are not hashed (key_is_bad, :392-425)."""
    lut = np.full(256, 255, dtype=np.uint8)
    for i, ch in enumerate(b"acgt"):
        lut[ch] = i
        lut[ord(chr(ch).upper())] = i
    codes, owner = [], []
    for iid in range(bgn, end + 1):
        r = iid - rs.first_iid
        if not loadable(r):
            continue
        b = lut[np.frombuffer(rs.read(r), dtype=np.uint8)]
        L = b.shape[0]
        if L < k:
            continue
        win = np.lib.stride_tricks.sliding_window_view(b, k)
        ok = (win != 255).all(axis=1)
        w = win[ok].astype(np.uint64)
        c = (w << (2 * np.arange(k, dtype=np.uint64))).sum(axis=1, dtype=np.uint64)
        codes.append(c)
        owner.append(np.full(c.shape[0], iid - bgn, dtype=np.int64))
    hist = np.zeros(end - bgn + 1, dtype=np.int64)
    if codes:
        allc = np.concatenate(codes)
        allo = np.concatenate(owner)
        _, first = np.unique(allc, return_index=True)
        hist += np.bincount(allo[first], minlength=hist.shape[0])
    return hist


def hash_batch_end(rs, params: dict, bgn: int, end: int, hashstrings: int, hashdatalen: int,
                   hashbits: int, hashload: float) -> int:
    """Build_Hash_Index's loading loop (overlapInCore-Build_Hash_Index.C:495-541): the last
    ID it loads from bgn on.  Raises where the reference asserts (:523)."""
    AS_MAX_READLEN = (1 << 21) - 1
    lens = rs.lengths
    minlen = params["min_olap_len"]
    loadable = lambda r: int(lens[r]) >= minlen
    max_alloc = sum(int(lens[i - rs.first_iid]) + 1 for i in range(bgn, end + 1)
                    if loadable(i - rs.first_iid))
    if max_alloc >= hashdatalen + AS_MAX_READLEN:
        raise ValueError("Build_Hash_Index.C:523 assert")
    limit = int(hashload * (1 << hashbits) * ENTRIES_PER_BUCKET)
    hist = first_read_kmers(rs, bgn, end, params["kmer_len"], loadable)
    strings = total = entries = 0
    cur = bgn
    while strings < hashstrings and total < hashdatalen and entries < limit and cur <= end:
        r = cur - rs.first_iid
        if loadable(r):
            total += int(lens[r]) + 1
            entries += int(hist[cur - bgn])
        cur += 1
        strings += 1
    return cur - 1


def run_oracle_driver(rs, params: dict, hash_range=(1, UINT32_MAX), ref_range=(1, UINT32_MAX),
                      threads: int = 1, hashstrings: int = 10000, hashdatalen: int = 100000000,
                      hashbits: int = 22, hashload: float = 0.6, skip_kmers=None,
                      with_stats=False):
    """OverlapDriver (overlapInCore.C:190-300) restated over the oracle: hash batches with
    Build_Hash_Index's loading rules, the `while (bgnHashID < endHashID)` loop (:222), and
    the ref reads Process_Overlaps' thread blocks actually search (:249-269,
    Process_Overlaps.C:86: a block starting at endRefID is skipped).  Counters add up over
    the batches."""
    nr = rs.first_iid + rs.nreads - 1
    gbh, geh = max(hash_range[0], 1), min(hash_range[1], nr)
    gbr, ger = max(ref_range[0], 1), min(ref_range[1], nr)
    ref_last = None
    if gbr < ger:
        per = 1 + (ger - gbr) // max(threads, 1) // 8
        ref_last = ger - 1 if (ger - gbr) % per == 0 else ger
    recs, tot, batches = [], None, []
    bgn, end = gbh, gbh + hashstrings - 1
    while bgn < geh:
        end = min(end, geh)
        end = hash_batch_end(rs, params, bgn, end, hashstrings, hashdatalen, hashbits, hashload)
        batches.append((bgn, end))
        if ref_last is not None:
            rec, st = run_oracle(rs, params, hash_range=(bgn, end), ref_range=(gbr, ref_last),
                                 skip_kmers=skip_kmers, with_stats=True)
            recs.append(rec)
            tot = st if tot is None else {f: tot[f] + st[f] for f in st}
        bgn, end = end + 1, end + hashstrings
    rec = sort_records(np.concatenate(recs)) if recs else np.zeros(0, dtype=RECORD_DTYPE)
    if tot is None:
        tot = {f: 0 for f, _ in OracleStats._fields_}
    tot["hash_batches"] = len(batches)
    if with_stats:
        return rec, tot, batches
    return rec


def run_reference(rs, params: dict, threads: int = 1, hash_bits: int = 20,
                  skip_kmers=None, minkmers: bool = False, extra=None, workdir=None,
                  with_time=False, batching: dict | None = None, with_stats=False,
                  libs=None, reads_path=None):
    """Run the reference overlapInCore (built from its sources) on `rs`.

    By default the whole read set is one hash batch and one ref range, so every pair (a<b)
    is searched once, as the reference's full -h/-r ranges do.  `batching` instead passes
    the hash-batch options as given ({"hashstrings": .., "hashdatalen": .., "hashload": ..},
    missing ones at the reference defaults, overlapInCore.H:447-450).  `libs` (one library
    number >= 1 per read) spreads the reads over gkpStore libraries for -H / -R."""
    from canu_amd.synth import write_reads_file  # input writer only
    if not reference_available():
        raise FileNotFoundError(REF_BIN)
    own = workdir is None
    wd = workdir or tempfile.mkdtemp(prefix="oicref_", dir=os.environ.get("TMPDIR", "/tmp"))
    try:
        # reads_path: a reads file written beforehand (rs is then None; read sets too large
        # to hold twice in host memory are written piecewise, tools/make_c4_chunk_digest.py)
        reads = reads_path or os.path.join(wd, "reads.bin")
        if reads_path is None:
            write_reads_file(reads, rs)
        out = os.path.join(wd, "records.bin")
        args = [REF_BIN, reads, os.path.join(wd, "w"), out, "-t", str(threads),
                "--hashbits", str(hash_bits), "--time"]
        if batching is None:
            args += ["--hashstrings", str(max(rs.nreads + 10, 1000)),
                     "--hashdatalen", str(rs.total_bases() + rs.nreads + 1024)]
        else:
            for opt in ("hashstrings", "hashdatalen", "hashload"):
                if opt in batching:
                    args += ["--" + opt, str(batching[opt])]
        args += params_to_ref_args(params)
        if minkmers:
            args.append("--minkmers")
        if skip_kmers:
            sk = os.path.join(wd, "skip.fasta")
            with open(sk, "w") as f:
                for i, k in enumerate(skip_kmers):
                    f.write(f">{i}\n{k if isinstance(k, str) else k.decode()}\n")
            args += ["--skip", sk]
        if libs is not None:
            lp = os.path.join(wd, "libs.bin")
            np.ascontiguousarray(libs, dtype="<u4").tofile(lp)
            args += ["--libs", lp]
        if extra:
            args += list(extra)
        t0 = time.time()
        cp = subprocess.run(args, capture_output=True, text=True)
        wall = time.time() - t0
        if cp.returncode != 0:
            raise RuntimeError(f"oic_ref failed ({cp.returncode}): {cp.stderr[-2000:]}")
        secs = None
        stats = {}
        for line in cp.stdout.splitlines():
            if line.startswith("OVERLAPDRIVER_SECONDS"):
                secs = float(line.split()[1])
            if line.startswith("STATS"):
                stats = {kv.split("=")[0]: int(kv.split("=")[1]) for kv in line.split()[1:]}
        rec = np.fromfile(out, dtype=RECORD_DTYPE)
        rec = sort_records(rec)
        if with_time:
            return rec, secs, wall
        if with_stats:
            return rec, stats
        return rec
    finally:
        if own:
            subprocess.run(["rm", "-rf", wd])
