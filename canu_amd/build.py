"""Build the gfx950 libraries in-tree (canu_amd/lib/) with hipcc and the drop-in executables over
them (canu_amd/bin/) with the host compiler."""
from __future__ import annotations

import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT_DIR = os.path.join(HERE, "lib")
OUT = os.path.join(OUT_DIR, "libcanu_ovl.so")
SOURCES = ["ovl_api.hip", "ovl_index.hip", "ovl_seed.hip", "ovl_extend.hip", "ovl_common.h",
           "ovl_ovb.h", "ovl_plan.h", "ped_host.h",
           # the host side, included by ovl_api.hip
           "ovl_ctx.h", "ovl_sq.hip", "ovl_build.hip", "ovl_find.hip", "ovl_driver.hip"]

HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
               # doubles in the extension (branch score, slope, quality) must round exactly
               # as the reference's: no fused multiply-add contraction
               "-ffp-contract=off"]

INCLUDE = os.path.join(HERE, "..", "include")
BIN_DIR = os.path.join(HERE, "bin")


def _csrc(*names: str) -> list:
    return [os.path.join(CSRC, n) for n in names]


def _inc(*names: str) -> list:
    return [os.path.join(INCLUDE, n) for n in names]


def _stale(out: str, deps: list) -> bool:
    return not os.path.exists(out) or \
        any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps)


def _run(cmd: list, out: str, verbose: bool) -> str:
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True, cwd=CSRC)
    os.replace(out + ".tmp", out)
    return out


def _hipcc_lib(out: str, src: str, deps: list, force: bool, verbose: bool, extra=()) -> str:
    """A shared library of one .hip file for gfx950, rebuilt when a dependency is newer."""
    if not force and not _stale(out, deps):
        return out
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return _run([hipcc, *HIPCC_FLAGS, *extra, "-o", out + ".tmp", os.path.join(CSRC, src)],
                out, verbose)


def _host_cli(out: str, src: str, lib, libname, deps: list, force: bool, verbose: bool,
              extra_libs=()) -> str:
    """A drop-in executable: host C++ over the library `lib` (lib<libname>.so), found next to
    it through the rpath; lib None: host only."""
    src = os.path.join(CSRC, src)
    if not force and not _stale(out, [src, *deps] + ([lib] if lib else [])):
        return out
    link = ["-L" + OUT_DIR, "-l" + libname, *extra_libs, "-Wl,-rpath,$ORIGIN/../lib",
            "-Wl,--allow-shlib-undefined"] if lib else []
    cxx = os.environ.get("CXX", "g++")
    return _run([cxx, "-O2", "-std=c++17", "-Wall", "-I" + INCLUDE, "-o", out + ".tmp", src, *link],
                out, verbose)


OVL_DEPS = _csrc(*SOURCES) + _inc("canu_ovl.h")
PROF_OUT = os.path.join(OUT_DIR, "libcanu_ovl_prof.so")
CLI_OUT = os.path.join(BIN_DIR, "overlapInCore")
CLI_DEPS = _csrc("oic_main.cpp", "gkp_store.h") + _inc("canu_ovl.h")

# the C-API scaffold of libcanu_mhap and the five libraries below meryl
CAPI_DEPS = _csrc("capi_common.h", "hip_raii.h")

MHAP_OUT = os.path.join(OUT_DIR, "libcanu_mhap.so")
MHAP_DEPS = _csrc("mhap.hip", "mhap_hash.h", "mhap_common.h", "mhap_sketch.hip", "mhap_filter.hip",
                  "mhap_host.h", "mhap_ctx.h") + CAPI_DEPS + _inc("canu_mhap.h", "canu_ovl.h")
MHAP_CLI_OUT = os.path.join(BIN_DIR, "mhap")

MERYL_OUT = os.path.join(OUT_DIR, "libcanu_meryl.so")
MERYL_DEPS = _csrc("meryl.hip", "meryl_host.h") + _inc("canu_meryl.h")
MERYL_CLI_OUT = os.path.join(BIN_DIR, "meryl")
EMT_CLI_OUT = os.path.join(BIN_DIR, "estimate-mer-threshold")

# the aligner pair.hip, fs.hip and gfa.hip share, and its host side
EDLIB_DEPS = _csrc("edlib_wave.h", "edlib_host.h", "edlib_launch.h") + CAPI_DEPS

PAIR_OUT = os.path.join(OUT_DIR, "libcanu_pair.so")
PAIR_DEPS = _csrc("pair.hip") + EDLIB_DEPS + _inc("canu_pair.h", "canu_ovl.h")
PAIR_CLI_OUT = os.path.join(BIN_DIR, "overlapPair")

# the aligner fe.hip and co.hip share, and its host side
PED_DEPS = _csrc("ped_wave.h", "ped_host.h", "ped_launch.h") + CAPI_DEPS
FE_OUT = os.path.join(OUT_DIR, "libcanu_fe.so")
FE_DEPS = _csrc("fe.hip") + PED_DEPS + _inc("canu_fe.h", "canu_ovl.h")
FE_CLI_OUT = os.path.join(BIN_DIR, "findErrors")

CO_OUT = os.path.join(OUT_DIR, "libcanu_co.so")
CO_DEPS = _csrc("co.hip") + PED_DEPS + _inc("canu_co.h", "canu_fe.h", "canu_ovl.h")
CO_CLI_OUT = os.path.join(BIN_DIR, "correctOverlaps")

FS_OUT = os.path.join(OUT_DIR, "libcanu_fs.so")
FS_DEPS = _csrc("fs.hip", "fs_fasta.h") + EDLIB_DEPS + _inc("canu_fs.h")
FS_CLI_OUT = os.path.join(BIN_DIR, "falconsense")

TR_OUT = os.path.join(OUT_DIR, "libcanu_tr.so")
TR_DEPS = _csrc("tr.hip") + CAPI_DEPS + _inc("canu_tr.h", "canu_ovl.h")
TR_CLI_OUT = os.path.join(BIN_DIR, "trimReads")

SR_OUT = os.path.join(OUT_DIR, "libcanu_sr.so")
SR_DEPS = _csrc("sr.hip") + CAPI_DEPS + _inc("canu_sr.h", "canu_ovl.h")
SR_CLI_OUT = os.path.join(BIN_DIR, "splitReads")

GFA_OUT = os.path.join(OUT_DIR, "libcanu_gfa.so")
GFA_DEPS = _csrc("gfa.hip", "gfa_host.h") + EDLIB_DEPS + _inc("canu_gfa.h")
GFA_CLI_OUT = os.path.join(BIN_DIR, "alignGFA")


def needs_build() -> bool:
    return _stale(OUT, OVL_DEPS)


def build(force: bool = False, verbose: bool = True, profile: bool = False) -> str:
    """libcanu_ovl.so.  profile=True builds the instrumented variant (in-kernel cycle stamps,
    OVL_DEBUG=1 prints them) as libcanu_ovl_prof.so; load it with CANU_OVL_LIB."""
    if profile:
        return _hipcc_lib(PROF_OUT, "ovl_api.hip", [], True, verbose, extra=["-DOVL_PROFILE"])
    return _hipcc_lib(OUT, "ovl_api.hip", OVL_DEPS, force, verbose)


def build_cli(force: bool = False, verbose: bool = True) -> str:
    """canu_amd/bin/overlapInCore: the overlapInCore-compatible executable."""
    return _host_cli(CLI_OUT, "oic_main.cpp", build(verbose=verbose), "canu_ovl", CLI_DEPS[1:],
                     force, verbose)


def build_mhap(force: bool = False, verbose: bool = True) -> str:
    """canu_amd/lib/libcanu_mhap.so: the MHAP stage."""
    return _hipcc_lib(MHAP_OUT, "mhap.hip", MHAP_DEPS, force, verbose)


def build_mhap_cli(force: bool = False, verbose: bool = True) -> str:
    """canu_amd/bin/mhap: the MHAP command line canu's mhap.sh / precompute.sh run (zlib for
    -f .gz)."""
    return _host_cli(MHAP_CLI_OUT, "mhap_main.cpp", build_mhap(verbose=verbose), "canu_mhap",
                     MHAP_DEPS[1:], force, verbose, extra_libs=["-lz"])


def build_meryl(force: bool = False, verbose: bool = True) -> str:
    """canu_amd/lib/libcanu_meryl.so: the k-mer count (meryl's frequent-mer step)."""
    return _hipcc_lib(MERYL_OUT, "meryl.hip", MERYL_DEPS, force, verbose)


def build_meryl_cli(force: bool = False, verbose: bool = True) -> str:
    """canu_amd/bin/meryl: the three meryl command lines canu's 0-mercounts stage runs."""
    return _host_cli(MERYL_CLI_OUT, "meryl_main.cpp", build_meryl(verbose=verbose), "canu_meryl",
                     _csrc("gkp_store.h") + MERYL_DEPS[1:], force, verbose)


def build_emt_cli(force: bool = False, verbose: bool = True) -> str:
    """canu_amd/bin/estimate-mer-threshold: host only, no library."""
    return _host_cli(EMT_CLI_OUT, "emt_main.cpp", None, None, [], force, verbose)


def build_pair(force: bool = False, verbose: bool = True) -> str:
    """canu_amd/lib/libcanu_pair.so: overlapPair, the exact realignment of MHAP overlaps."""
    return _hipcc_lib(PAIR_OUT, "pair.hip", PAIR_DEPS, force, verbose)


def build_pair_cli(force: bool = False, verbose: bool = True) -> str:
    """canu_amd/bin/overlapPair: the command line canu's mhap.sh runs after mhapConvert."""
    return _host_cli(PAIR_CLI_OUT, "pair_main.cpp", build_pair(verbose=verbose), "canu_pair",
                     _csrc("gkp_store.h", "ovl_ovb.h", "ovb_reader.h") + _inc("canu_pair.h", "canu_ovl.h"),
                     force, verbose)


def build_fe(force: bool = False, verbose: bool = True) -> str:
    """canu_amd/lib/libcanu_fe.so: findErrors, read error detection from the overlaps."""
    return _hipcc_lib(FE_OUT, "fe.hip", FE_DEPS, force, verbose)


def build_fe_cli(force: bool = False, verbose: bool = True) -> str:
    """canu_amd/bin/findErrors: the command line canu's red.sh runs."""
    return _host_cli(FE_CLI_OUT, "fe_main.cpp", build_fe(verbose=verbose), "canu_fe",
                     _csrc("gkp_store.h", "ovs_reader.h") + _inc("canu_fe.h", "canu_ovl.h"),
                     force, verbose)


def build_co(force: bool = False, verbose: bool = True) -> str:
    """canu_amd/lib/libcanu_co.so: correctOverlaps, overlap error rates from corrected reads."""
    return _hipcc_lib(CO_OUT, "co.hip", CO_DEPS, force, verbose)


def build_co_cli(force: bool = False, verbose: bool = True) -> str:
    """canu_amd/bin/correctOverlaps: the command line canu's oea.sh runs."""
    return _host_cli(CO_CLI_OUT, "co_main.cpp", build_co(verbose=verbose), "canu_co",
                     _csrc("gkp_store.h", "ovs_reader.h", "co_files.h") +
                     _inc("canu_co.h", "canu_fe.h", "canu_ovl.h"), force, verbose)


def build_fs(force: bool = False, verbose: bool = True) -> str:
    """canu_amd/lib/libcanu_fs.so: falconsense, corrected reads from correction layouts."""
    return _hipcc_lib(FS_OUT, "fs.hip", FS_DEPS, force, verbose)


def build_fs_cli(force: bool = False, verbose: bool = True) -> str:
    """canu_amd/bin/falconsense: the command line canu's correctReads.sh runs."""
    return _host_cli(FS_CLI_OUT, "fs_main.cpp", build_fs(verbose=verbose), "canu_fs",
                     _csrc("gkp_store.h", "tgs_reader.h", "fs_fasta.h") + _inc("canu_fs.h"),
                     force, verbose)


def build_tr(force: bool = False, verbose: bool = True) -> str:
    """canu_amd/lib/libcanu_tr.so: trimReads, overlap based trimming from the overlaps."""
    return _hipcc_lib(TR_OUT, "tr.hip", TR_DEPS, force, verbose)


def build_tr_cli(force: bool = False, verbose: bool = True) -> str:
    """canu_amd/bin/trimReads: the command line canu's trimming stage runs."""
    return _host_cli(TR_CLI_OUT, "tr_main.cpp", build_tr(verbose=verbose), "canu_tr",
                     _csrc("gkp_store.h", "ovs_reader.h", "tr_files.h") +
                     _inc("canu_tr.h", "canu_ovl.h"), force, verbose)


def build_sr(force: bool = False, verbose: bool = True) -> str:
    """canu_amd/lib/libcanu_sr.so: splitReads, subread detection and read splitting."""
    return _hipcc_lib(SR_OUT, "sr.hip", SR_DEPS, force, verbose)


def build_sr_cli(force: bool = False, verbose: bool = True) -> str:
    """canu_amd/bin/splitReads: the command line canu's trimming stage runs after trimReads."""
    return _host_cli(SR_CLI_OUT, "sr_main.cpp", build_sr(verbose=verbose), "canu_sr",
                     _csrc("gkp_store.h", "ovs_reader.h", "tr_files.h", "sr_files.h") +
                     _inc("canu_sr.h", "canu_ovl.h"), force, verbose)


def build_gfa(force: bool = False, verbose: bool = True) -> str:
    """canu_amd/lib/libcanu_gfa.so: alignGFA, graph links and unitig positions realigned."""
    return _hipcc_lib(GFA_OUT, "gfa.hip", GFA_DEPS, force, verbose)


def build_gfa_cli(force: bool = False, verbose: bool = True) -> str:
    """canu_amd/bin/alignGFA: the command line canu runs on its graphs after consensus."""
    return _host_cli(GFA_CLI_OUT, "gfa_main.cpp", build_gfa(verbose=verbose), "canu_gfa",
                     _csrc("gfa_files.h", "gfa_host.h", "tgs_reader.h") + _inc("canu_gfa.h"),
                     force, verbose)


if __name__ == "__main__":
    force = "--force" in sys.argv
    build(force=force, profile="--profile" in sys.argv)
    if "--profile" not in sys.argv:
        for f in (build_mhap, build_cli, build_meryl, build_meryl_cli, build_emt_cli, build_pair,
                  build_pair_cli, build_fe, build_fe_cli, build_co, build_co_cli, build_fs,
                  build_fs_cli, build_tr, build_tr_cli, build_sr, build_sr_cli, build_gfa,
                  build_gfa_cli):
            f(force=force)
