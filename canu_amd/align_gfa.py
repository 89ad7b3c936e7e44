"""canu's alignGFA (the realignment of graph links and unitig placements after consensus) over
the MI355X C-ABI (include/canu_gfa.h): src/gfa/alignGFA.C.

`AlignGFA.check_links` runs checkLink for every link of a GFA and returns every intermediate
coordinate, the three distances and the CIGAR; `check_records` runs checkRecord for every
placement of a BED and returns the new coordinates with the log of every try.  The alignments
and the paths run in libcanu_gfa.so on a gfx950 device; there is no CPU fallback.  The text
helpers build the program's output file and its stderr (plain and -V) from those results.
"""
from __future__ import annotations

import ctypes
import dataclasses
import os
import re

import numpy as np

from . import _capi

LIB_PATH = _capi.lib_path("gfa")

GFA_STATUS = {0: "GFA_OK", -1: "GFA_ERR_NO_DEVICE", -2: "GFA_ERR_BAD_PARAM",
              -3: "GFA_ERR_UNSUPPORTED", -4: "GFA_ERR_BAD_INPUT", -5: "GFA_ERR_HIP",
              -6: "GFA_ERR_OOM", -7: "GFA_ERR_STATE"}

ABI_VERSION = 1                         # GFA_ABI_VERSION of include/canu_gfa.h
SET_T, SET_C = 0, 1                     # GFA_SET_*
END_BASES = 50000                       # GFA_END_BASES
LEAF_BYTES = 1048576                    # GFA_LEAF_BYTES
MIN_OLAP = 100                          # alignGFA.C:725
CALLS = ("ALL", "LEFT", "RIGHT")        # GFA_CALL_*
ACCEPT, EXTEND, RELAX, ABORT = 0, 1, 2, 3   # GFA_TRY_*
U32MAX = 0xFFFFFFFF

LINK_DTYPE = np.dtype([("a_id", "<u4"), ("a_fwd", "<u4"), ("b_id", "<u4"), ("b_fwd", "<u4"),
                       ("a_align", "<i4"), ("b_align", "<i4"), ("align", "<i4")])
LINK_RESULT_DTYPE = np.dtype(
    [("success", "<i4"), ("max_edit", "<i4"), ("a_len", "<i4"), ("b_len", "<i4"),
     ("abgn_b", "<i4"), ("bend_b", "<i4"), ("dist_b", "<i4"), ("bend", "<i4"), ("abgn_a", "<i4"),
     ("dist_a", "<i4"), ("abgn", "<i4"), ("dist_f", "<i4"), ("align_len", "<i4"),
     ("n_runs", "<u4"), ("run_off", "<u8"), ("n_leaves", "<u4"), ("n_splits", "<u4")])
RUN_DTYPE = np.dtype([("count", "<u4"), ("op", "<u4")])
RECORD_DTYPE = np.dtype([("a_id", "<u4"), ("b_id", "<u4"), ("b_fwd", "<u4"), ("bgn", "<i4"),
                         ("end", "<i4")])
RECORD_RESULT_DTYPE = np.dtype([("success", "<i4"), ("bgn", "<i4"), ("end", "<i4"),
                                ("n_tries", "<u4"), ("try_off", "<u8")])
TRY_DTYPE = np.dtype([("record", "<u4"), ("call", "<u4"), ("b_len", "<i4"), ("abgn", "<i4"),
                      ("aend", "<i4"), ("max_edit", "<i4"), ("dist", "<i4"), ("nbgn", "<i4"),
                      ("nend", "<i4"), ("outcome", "<i4")])


class GfaError(_capi.CapiError):
    STATUS = GFA_STATUS


class _Params(ctypes.Structure):
    _fields_ = [("hbm_budget", ctypes.c_uint64)]


_STAT_U64 = ("n_links", "n_records", "n_alignments", "dp_cells", "n_passes", "n_rounds", "n_leaves",
             "n_splits", "n_batches", "scratch_bytes")
_STAT_F64 = ("ms_extend_b", "ms_extend_a", "ms_final", "ms_records")


class _Stats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in _STAT_U64] + [(n, ctypes.c_double) for n in _STAT_F64]


# Every symbol include/canu_gfa.h declares.
EXPORTS = ["gfa_params_init", "gfa_last_error", "gfa_abi_version", "gfa_ctx_create",
           "gfa_ctx_destroy", "gfa_set_params", "gfa_load_tigs", "gfa_check_links", "gfa_runs_size",
           "gfa_fetch_runs", "gfa_check_records", "gfa_tries_size", "gfa_fetch_tries",
           "gfa_get_stats"]

_lib = None


def load_library(path: str | None = None):
    """Load libcanu_gfa.so.  Raises if it was not built -- there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get("CANU_GFA_LIB") or LIB_PATH
    lib = _capi.load("gfa", path, ABI_VERSION, GfaError, _Params, _Stats, reads=False)
    V, U64, P = ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER
    lib.gfa_load_tigs.argtypes = [V, ctypes.c_int, ctypes.c_uint32, V, V, V]
    lib.gfa_check_links.argtypes = [V, V, U64, V]
    lib.gfa_runs_size.argtypes = [V, P(U64)]
    lib.gfa_fetch_runs.argtypes = [V, V]
    lib.gfa_check_records.argtypes = [V, V, U64, V]
    lib.gfa_tries_size.argtypes = [V, P(U64)]
    lib.gfa_fetch_tries.argtypes = [V, V]
    _lib = lib
    return lib


@dataclasses.dataclass
class GfaParameters:
    hbm_budget: int = 0                 # bytes of per-link / per-record buffers per batch; 0: 4 GiB

    def to_c(self) -> _Params:
        return _Params(int(self.hbm_budget))


class AlignGFA(_capi.Context):
    """One alignGFA job on one gfx950 device: load the tigs, check links or records."""
    PREFIX, ERROR, PARAMS, STATS = "gfa", GfaError, GfaParameters, _Stats

    def __init__(self, params: GfaParameters | None = None, device: int = 0):
        super().__init__(load_library(), params, device)

    def load_tigs(self, which: int, tigs: list) -> None:
        """tigs[i] is the ungapped sequence of tig i as bytes (b"" or None: deleted)."""
        tigs = [t or b"" for t in tigs]
        lens = np.array([len(t) for t in tigs], dtype=np.uint32)
        offs = np.zeros(len(tigs), dtype=np.uint64)
        if len(tigs) > 1:
            offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
        bases = np.frombuffer(b"".join(tigs) or b"\0", dtype=np.uint8)
        self._check(self.lib.gfa_load_tigs(self.ctx, which, len(tigs), bases.ctypes.data,
                                           offs.ctypes.data if len(tigs) else None,
                                           lens.ctypes.data if len(tigs) else None))

    def check_links(self, links: np.ndarray):
        """links: LINK_DTYPE records.  -> (LINK_RESULT_DTYPE results, RUN_DTYPE runs): link i's
        CIGAR is runs[run_off : run_off + n_runs]."""
        lk = np.ascontiguousarray(links, dtype=LINK_DTYPE)
        res = np.zeros(lk.shape[0], dtype=LINK_RESULT_DTYPE)
        self._check(self.lib.gfa_check_links(self.ctx, lk.ctypes.data if lk.size else None,
                                             lk.shape[0], res.ctypes.data if lk.size else None))
        n = ctypes.c_uint64()
        self._check(self.lib.gfa_runs_size(self.ctx, ctypes.byref(n)))
        runs = np.zeros(n.value, dtype=RUN_DTYPE)
        self._check(self.lib.gfa_fetch_runs(self.ctx, runs.ctypes.data if n.value else None))
        return res, runs

    def check_records(self, records: np.ndarray):
        """records: RECORD_DTYPE records.  -> (RECORD_RESULT_DTYPE results, TRY_DTYPE tries)."""
        rc = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
        res = np.zeros(rc.shape[0], dtype=RECORD_RESULT_DTYPE)
        self._check(self.lib.gfa_check_records(self.ctx, rc.ctypes.data if rc.size else None,
                                               rc.shape[0], res.ctypes.data if rc.size else None))
        n = ctypes.c_uint64()
        self._check(self.lib.gfa_tries_size(self.ctx, ctypes.byref(n)))
        tries = np.zeros(n.value, dtype=TRY_DTYPE)
        self._check(self.lib.gfa_fetch_tries(self.ctx, tries.ctypes.data if n.value else None))
        return res, tries


# ------------------------------------------------------------------ the files

def _strtoll(s: str) -> int:
    m = re.match(r"\s*([+-]?\d+)", s)
    return int(m.group(1)) if m else 0


def name_to_id(name: str) -> int:
    """nameToCanuID: 'tig', 'utg' or 'ctg' and a number; anything else is UINT32_MAX."""
    if name[:3] in ("tig", "utg", "ctg"):
        return _strtoll(name[3:]) & U32MAX
    return U32MAX


def cigar_lengths(cigar: str) -> tuple[int, int, int, list]:
    """gfaLink::alignmentLength -> (a_align, b_align, align, the warnings it prints)."""
    q = r = a = 0
    warn = []
    if cigar.startswith("*"):
        return q, r, a, warn
    pos = 0
    while True:
        m = re.match(r"\s*[+-]?\d+", cigar[pos:])
        val = int(m.group(0)) if m else 0
        pos += m.end() if m else 0
        code = cigar[pos:pos + 1]
        pos += 1
        if code in ("M", "=", "X"):
            r += val; q += val; a += val
        elif code == "I":
            q += val; a += val
        elif code == "D":
            r += val; a += val
        elif code in ("N", "S", "H", "P"):
            r += val if code == "N" else 0
            warn.append(f"warning - unsupported CIGAR code '{code}' in '{cigar}'\n")
        else:
            warn.append(f"unknown CIGAR code '{code}' in '{cigar}'\n")
        if pos >= len(cigar):
            break
    return q, r, a, warn


def parse_gfa(text: str) -> dict:
    """-> {header, sequences [(name, sequence field, id)], links [(Aname, Afwd, Bname, Bfwd,
    cigar)], array (LINK_DTYPE), warnings (per link)}."""
    header, seqs, links = None, [], []
    for line in text.split("\n"):
        if line == "":
            continue
        if len(line) < 2 or line[1] != "\t":
            raise ValueError(f"misformed line '{line}'")
        w = line.split()
        if line[0] == "H":
            header = line[2:]
        elif line[0] == "S":
            if len(w) < 4:
                raise ValueError(f"S line with {len(w)} fields")
            seqs.append((w[1], w[2], name_to_id(w[1])))
        elif line[0] == "L":
            if len(w) < 6:
                raise ValueError(f"L line with {len(w)} fields")
            links.append((w[1], w[2][0] == "+", w[3], w[4][0] == "+", w[5]))
        else:
            raise ValueError(f"unrecognized line '{line}'")
    arr = np.zeros(len(links), dtype=LINK_DTYPE)
    warnings = []
    for i, (an, af, bn, bf, cg) in enumerate(links):
        q, r, a, warn = cigar_lengths(cg)
        arr[i] = (name_to_id(an), af, name_to_id(bn), bf, q, r, a)
        warnings.append(warn)
    return {"header": header, "sequences": seqs, "links": links, "array": arr, "warnings": warnings}


def parse_bed(text: str) -> dict:
    """-> {records [(Aname, bgn, end, Bname, score, Bfwd)], array (RECORD_DTYPE)}."""
    recs = []
    for line in text.split("\n"):
        if line == "":
            continue
        w = line.split()
        if len(w) < 6:
            raise ValueError(f"BED line with {len(w)} fields")
        recs.append((w[0], _strtoll(w[1]), _strtoll(w[2]), w[3], _strtoll(w[4]) & U32MAX,
                     w[5][0] == "+"))
    arr = np.zeros(len(recs), dtype=RECORD_DTYPE)
    for i, (an, b, e, bn, _, fwd) in enumerate(recs):
        arr[i] = (name_to_id(an), name_to_id(bn), fwd, b, e)
    return {"records": recs, "array": arr}


def bed_links(bed: dict):
    """The links processBEDtoGFA infers from the placements, in -t 1 order: every pair on one
    contig whose spans intersect by MIN_OLAP or more, '+ / +', with the overlap length its two
    ifs leave.  -> (links as parse_gfa's, array, used tig IDs)."""
    recs, arr = bed["records"], bed["array"]
    links, used = [], set()
    for ii in range(len(recs)):
        for jj in range(ii + 1, len(recs)):
            a, b = recs[ii], recs[jj]
            if arr[ii]["a_id"] != arr[jj]["a_id"]:
                continue
            if a[2] < b[1] + MIN_OLAP or b[2] < a[1] + MIN_OLAP:
                continue
            olap = 0
            if a[1] < b[2]:
                olap = a[2] - b[1]
            if b[1] < a[2]:
                olap = b[2] - a[1]
            if olap <= 0:
                raise ValueError("an overlap of no length")
            links.append((a[3], True, b[3], True, "%dM" % olap))
            used |= {int(arr[ii]["b_id"]), int(arr[jj]["b_id"])}
    out = np.zeros(len(links), dtype=LINK_DTYPE)
    for i, (an, _, bn, _, cg) in enumerate(links):
        n = int(cg[:-1])
        out[i] = (name_to_id(an), 1, name_to_id(bn), 1, n, n, n)
    return links, out, sorted(used)


def cigar_text(runs: np.ndarray) -> str:
    return "".join("%d%c" % (int(r["count"]), int(r["op"])) for r in runs)


def _sign(fwd) -> str:
    return "+" if fwd else "-"


def link_log(lk, r) -> str:
    """checkLink's -V lines for one link."""
    a, b, sa, sb = int(lk["a_id"]), int(lk["b_id"]), _sign(lk["a_fwd"]), _sign(lk["b_fwd"])
    alen = int(r["a_len"])
    out = ["LINK tig%08u %c %17s    tig%08u %c %17s   Aalign %6u Balign %6u align %6u\n"
           % (a, sa, "", b, sb, "", lk["a_align"], lk["b_align"], lk["align"])]
    row = "tig%08u %c %8d-%-8d    tig%08u %c %8d-%-8d"
    out.append(("TEST " + row + "  maxEdit=%6d  (extend B)")
               % (a, sa, r["abgn_b"], alen, b, sb, 0, r["bend_b"], r["max_edit"]))
    out.append("\n" if r["dist_b"] >= 0 else " - FAILED\n")
    out.append(("     " + row + "  maxEdit=%6d  (extend A)")
               % (a, sa, r["abgn_a"], alen, b, sb, 0, r["bend"], r["max_edit"]))
    out.append("\n" if r["dist_a"] >= 0 else " - FAILED\n")
    out.append(("     " + row + "  maxEdit=%6d  (final)")
               % (a, sa, r["abgn"], alen, b, sb, 0, r["bend"], r["max_edit"]))
    out.append("\n" if r["success"] else " - FAILED\n")
    dist, alen_f = (int(r["dist_f"]), int(r["align_len"])) if r["success"] else (0, int(lk["align"]))
    ratio = dist / alen_f if alen_f else float("nan")
    out.append(("     " + row + "   %.4f\n") % (a, sa, r["abgn"], alen, b, sb, 0, r["bend"], ratio))
    out.append("\n")
    return "".join(out)


def _save_gfa(header: str, seqs: list, links: list, cigars: list, keep_failed: bool) -> str:
    out = ["H\t%s\n" % header]
    out += ["S\t%s\t%s\tLN:i:%u\n" % s for s in seqs]
    for (an, af, bn, bf, _), cg in zip(links, cigars):
        if cg is not None or keep_failed:
            out.append("L\t%s\t%c\t%s\t%c\t%s\n" % (an, _sign(af), bn, _sign(bf),
                                                    "*" if cg is None else cg))
    return "".join(out)


def _cigars(res, runs) -> list:
    return [cigar_text(runs[int(r["run_off"]):int(r["run_off"]) + int(r["n_runs"])])
            if r["success"] else None for r in res]


def gfa_output(gfa: dict, tig_lengths, res, runs, names: dict, verbose: bool):
    """processGFA's output file and stderr from check_links' results."""
    L, arr = gfa["links"], gfa["array"]
    err = ["-- Reading GFA '%s'.\n" % names["in"],
           "gfa:  Loaded %d sequences and %d links.\n" % (len(gfa["sequences"]), len(L)),
           "-- Loading sequences from tigStore '%s' version %u.\n" % (names["T"], names["Tv"]),
           "-- Resetting sequence lengths.\n",
           "-- Aligning %u links using %u threads.\n" % (len(L), 1)]
    pc = fc = pn = fn = 0
    for i, (an, af, bn, bf, _) in enumerate(L):
        lk, r = arr[i], res[i]
        circ = lk["a_id"] == lk["b_id"]
        if circ:
            if verbose:
                err.append("Processing circular link for tig %u\n" % lk["a_id"])
            if af != bf:
                err.append("WARNING: %s %c %s %c -- circular to the same end!?\n"
                           % (an, _sign(af), bn, _sign(bf)))
        elif verbose:
            err.append("Processing link between tig %u %s and tig %u %s\n"
                       % (lk["a_id"], "-->" if af else "<--", lk["b_id"], "-->" if bf else "<--"))
        err += gfa["warnings"][i]
        if verbose:
            err.append(link_log(lk, r))
            if not r["success"]:
                err.append("  Failed to find alignment.\n")
        ok = bool(r["success"])
        if circ:
            pc, fc = pc + ok, fc + (not ok)
        else:
            pn, fn = pn + ok, fn + (not ok)
    seqs = [(n, s, int(tig_lengths[i])) for (n, s, i) in gfa["sequences"]]
    out = _save_gfa(gfa["header"], seqs, L, _cigars(res, runs), False)
    err += ["-- Writing GFA '%s'.\n" % names["out"], "-- Cleaning up.\n",
            "-- Aligned %6u ciruclar tigs, failed %6u\n" % (pc, fc),
            "-- Aligned %6u   linear tigs, failed %6u\n" % (pn, fn), "Bye.\n"]
    return out, "".join(err)


def try_log(t, aname: str, bname: str, alen: int) -> str:
    """checkRecord_align's -V line for one try."""
    out = "ALIGN %5s utg %s len=%7d to ctg %s %9d-%9d len=%9d" % (
        CALLS[int(t["call"])], bname, t["b_len"], aname, t["abgn"], t["aend"], alen)
    if t["dist"] >= 0:
        d = int(t["dist"])
        alen_ = ((int(t["nend"]) - int(t["nbgn"])) + int(t["b_len"]) + d) // 2
        score = 1000 - int(1000.0 * d / alen_)
        return out + " - POSITION from %9d-%-9d to %9d-%-9d score %5d/%9d = %4d\n" % (
            t["abgn"], t["aend"], t["nbgn"], t["nend"], d, alen_, score)
    return out + (" - FAILED, RELAX\n" if t["outcome"] == RELAX else " - ABORT, ABORT, ABORT!\n")


def bed_output(bed: dict, ctg_lengths, res, tries, names: dict, verbose: bool):
    """processBED's output file and stderr from check_records' results."""
    recs, arr = bed["records"], bed["array"]
    err = ["-- Reading BED '%s'.\n" % names["in"], "bed:  Loaded %d records.\n" % len(recs),
           "-- Loading sequences from tigStore '%s' version %u.\n" % (names["T"], names["Tv"]),
           "-- Loading sequences from tigStore '%s' version %u.\n" % (names["C"], names["Cv"]),
           "-- Aligning %u records using %u threads.\n" % (len(recs), 1)]
    out = []
    npass = 0
    for i, (an, b, e, bn, score, fwd) in enumerate(recs):
        r = res[i]
        if verbose:
            alen = int(ctg_lengths[int(arr[i]["a_id"])])
            for t in tries[int(r["try_off"]):int(r["try_off"]) + int(r["n_tries"])]:
                err.append(try_log(t, an, bn, alen))
        if r["success"]:
            npass += 1
            out.append("%s\t%d\t%d\t%s\t%u\t%c\n" % (an, r["bgn"], r["end"], bn, 0, _sign(fwd)))
    err += ["-- Writing BED '%s'.\n" % names["out"], "-- Cleaning up.\n",
            "-- Aligned %6u unitigs to contigs, failed %6u\n" % (npass, len(recs) - npass), "Bye.\n"]
    return "".join(out), "".join(err)


def bed_gfa_output(bed: dict, links: list, arr, used: list, tig_lengths, res, runs, names: dict,
                   verbose: bool):
    """processBEDtoGFA's output file and stderr from check_links' results on bed_links."""
    err = ["-- Loading sequences from tigStore '%s' version %u.\n" % (names["T"], names["Tv"]),
           "-- Reading BED '%s'.\n" % names["in"],
           "bed:  Loaded %d records.\n" % len(bed["records"]),
           "-- Aligning %u records using %u threads.\n" % (len(bed["records"]), 1)]
    if verbose:
        err += [link_log(arr[i], res[i]) for i in range(len(links))]
    seqs = [("utg%08u" % i, "*", int(tig_lengths[i])) for i in used]
    out = _save_gfa("H\tVN:Z:bogart/edges", seqs, links, _cigars(res, runs), True)
    err.append("Bye.\n")
    return out, "".join(err)


def parse_alignGFA_args(argv: list) -> dict:
    """alignGFA's command line: -T t v, -C t v, -gfa, -bed, -i, -o, -V, -t.  Anything else, a
    missing -T / -i / -o or a version 0 raises ValueError, where the program exits with 1."""
    o = {"T": None, "Tv": U32MAX, "C": None, "Cv": U32MAX, "type": "gfa", "in": None, "out": None,
         "verbose": 0, "threads": None}
    i, bad = 0, []
    while i < len(argv):
        a = argv[i]
        if a in ("-T", "-C") and i + 2 < len(argv):
            o[a[1]] = argv[i + 1]
            o[a[1] + "v"] = _capi._atoi(argv[i + 2]) & U32MAX
            i += 2
        elif a in ("-gfa", "-bed"):
            o["type"] = a[1:]
        elif a in ("-i", "-o") and i + 1 < len(argv):
            o["in" if a == "-i" else "out"] = argv[i + 1]
            i += 1
        elif a == "-V":
            o["verbose"] += 1
        elif a == "-t" and i + 1 < len(argv):
            o["threads"] = _capi._atoi(argv[i + 1])
            i += 1
        else:
            bad.append(a)
        i += 1
    if bad:
        raise ValueError(f"unknown option '{bad[0]}'")
    for k, what in (("T", "no tigStore (-T)"), ("in", "no input (-i)"), ("out", "no output (-o)")):
        if o[k] is None:
            raise ValueError(what + " supplied")
    if o["Tv"] == 0 or (o["C"] is not None and o["Cv"] == 0):
        raise ValueError("invalid tigStore version supplied")
    return o


def run_program(gfa: AlignGFA, argv: list, tigs_T: list, tigs_C: list | None, text: str):
    """What the alignGFA program does with these arguments: -> (output file, stderr)."""
    o = parse_alignGFA_args(argv)
    lens_T = [len(t or b"") for t in tigs_T]
    gfa.load_tigs(SET_T, tigs_T)
    v = o["verbose"] > 0
    if o["type"] == "gfa":
        g = parse_gfa(text)
        for (name, _, tid) in g["sequences"]:
            if tid >= len(tigs_T):
                raise GfaError(-4, f"sequence {name} is outside the store")
        res, runs = gfa.check_links(g["array"])
        return gfa_output(g, lens_T, res, runs, o, v)
    b = parse_bed(text)
    if o["C"] is not None:
        gfa.load_tigs(SET_C, tigs_C)
        res, tries = gfa.check_records(b["array"])
        return bed_output(b, [len(t or b"") for t in tigs_C], res, tries, o, v)
    links, arr, used = bed_links(b)
    res, runs = gfa.check_links(arr)
    return bed_gfa_output(b, links, arr, used, lens_T, res, runs, o, v)


# ------------------------------------------------------------------ synthetic jobs

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _mutate(rng, seq: np.ndarray, rate: float) -> bytes:
    """Substitutions, insertions and deletions at `rate`, a third each."""
    n = seq.shape[0]
    hit = rng.random(n) < rate
    kind = rng.integers(0, 3, n)
    sub = _ACGT[rng.integers(0, 4, n)]
    out = bytearray()
    last = 0
    for p in np.nonzero(hit)[0]:
        p = int(p)
        out += seq[last:p].tobytes()
        if kind[p] == 0:
            out.append(int(sub[p]))
        elif kind[p] == 1:
            out.append(int(seq[p]))
            out.append(int(sub[p]))
        last = p + 1
    out += seq[last:].tobytes()
    return bytes(out)


def synth_graph(seed: int = 1, n_links: int = 512, n_records: int = 64, tig_len: int = 12000,
                overlap: int = 2000, error_rate: float = 0.01, false_every: int = 8,
                ctg_len: int = 60000, utg_len: int = 6000) -> dict:
    """A graph cut from one random genome.  n_links + 1 unitigs of tig_len bases tile it with
    `overlap` bases between neighbours, each with its own errors and a random orientation; link
    i joins unitigs i and i + 1 in the orientation that is true, except every false_every-th,
    which joins i to a tig far away (a false overlap).  n_records further unitigs of utg_len
    bases are placed on contigs of ctg_len bases, within +-2 % of where they lie, every
    false_every-th 40 % of its length off (RELAX).
    -> {utgs, ctgs, links (LINK_DTYPE), records (RECORD_DTYPE), gfa_text, bed_text}."""
    rng = np.random.default_rng(seed)
    step = tig_len - overlap
    genome = _ACGT[rng.integers(0, 4, step * (n_links + 1) + overlap)]
    utgs, fwd = [], []
    for i in range(n_links + 1):
        s = _mutate(rng, genome[i * step:i * step + tig_len], error_rate)
        f = bool(rng.integers(0, 2))
        utgs.append(s if f else s.translate(_COMP)[::-1])
        fwd.append(f)
    links = np.zeros(n_links, dtype=LINK_DTYPE)
    for i in range(n_links):
        j = i + 1
        if false_every and i % false_every == false_every - 1:
            j = (i + n_links // 2 + 1) % (n_links + 1)
        links[i] = (i, fwd[i], j, fwd[j], overlap, overlap, overlap)
    n_ctg = max(1, (n_records * utg_len) // ctg_len)
    ctgs = [_ACGT[rng.integers(0, 4, ctg_len)].tobytes() for _ in range(n_ctg)]
    records = np.zeros(n_records, dtype=RECORD_DTYPE)
    first_rec = len(utgs)
    for k in range(n_records):
        c = k % n_ctg
        at = int(rng.integers(0, ctg_len - utg_len))
        s = _mutate(rng, np.frombuffer(ctgs[c][at:at + utg_len], dtype=np.uint8), error_rate)
        f = bool(rng.integers(0, 2))
        utgs.append(s if f else s.translate(_COMP)[::-1])
        off = int(rng.integers(-utg_len // 50, utg_len // 50 + 1))
        if false_every and k % false_every == false_every - 1:
            off = (2 * utg_len) // 5
        b = min(max(at + off, 0), ctg_len - utg_len)
        records[k] = (c, first_rec + k, f, b, b + utg_len)
    gfa_text = "H\tVN:Z:bogart/edges\n" + \
        "".join("S\ttig%08d\t*\tLN:i:%d\n" % (i, len(u)) for i, u in enumerate(utgs)) + \
        "".join("L\ttig%08d\t%s\ttig%08d\t%s\t%dM\n" % (l["a_id"], _sign(l["a_fwd"]), l["b_id"],
                                                      _sign(l["b_fwd"]), l["align"]) for l in links)
    bed_text = "".join("ctg%08d\t%d\t%d\tutg%08d\t0\t%s\n" % (r["a_id"], r["bgn"], r["end"],
                                                            r["b_id"], _sign(r["b_fwd"]))
                       for r in records)
    return {"utgs": utgs, "ctgs": ctgs, "links": links, "records": records, "gfa_text": gfa_text,
            "bed_text": bed_text}
