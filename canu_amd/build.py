"""Build libcanu_ovl.so (overlapInCore) and libcanu_mhap.so (MHAP stage) for gfx950 in-tree
(canu_amd/lib/) with hipcc."""
from __future__ import annotations

import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT_DIR = os.path.join(HERE, "lib")
OUT = os.path.join(OUT_DIR, "libcanu_ovl.so")
SOURCES = ["ovl_api.hip", "ovl_index.hip", "ovl_seed.hip", "ovl_extend.hip", "ovl_common.h",
           "ovl_ovb.h", "ovl_plan.h"]

HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
               # doubles in the extension (branch score, slope, quality) must round exactly
               # as the reference's: no fused multiply-add contraction
               "-ffp-contract=off"]


def needs_build() -> bool:
    if not os.path.exists(OUT):
        return True
    t = os.path.getmtime(OUT)
    deps = [os.path.join(CSRC, s) for s in SOURCES]
    deps.append(os.path.join(HERE, "..", "include", "canu_ovl.h"))
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


PROF_OUT = os.path.join(OUT_DIR, "libcanu_ovl_prof.so")
MHAP_OUT = os.path.join(OUT_DIR, "libcanu_mhap.so")
MHAP_DEPS = [os.path.join(CSRC, "mhap.hip"), os.path.join(HERE, "..", "include", "canu_mhap.h")]


def build_mhap(force: bool = False, verbose: bool = True) -> str:
    if not force and os.path.exists(MHAP_OUT) and \
            all(os.path.getmtime(d) <= os.path.getmtime(MHAP_OUT) for d in MHAP_DEPS):
        return MHAP_OUT
    os.makedirs(OUT_DIR, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, *HIPCC_FLAGS, "-o", MHAP_OUT + ".tmp", os.path.join(CSRC, "mhap.hip")]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True, cwd=CSRC)
    os.replace(MHAP_OUT + ".tmp", MHAP_OUT)
    return MHAP_OUT


BIN_DIR = os.path.join(HERE, "bin")
CLI_OUT = os.path.join(BIN_DIR, "overlapInCore")
CLI_DEPS = [os.path.join(CSRC, "oic_main.cpp"), os.path.join(CSRC, "gkp_store.h"),
            os.path.join(HERE, "..", "include", "canu_ovl.h")]


def build_cli(force: bool = False, verbose: bool = True) -> str:
    """canu_amd/bin/overlapInCore: the overlapInCore-compatible executable (host C++ over
    libcanu_ovl.so, found next to it through the rpath)."""
    lib = build(verbose=verbose)
    if not force and os.path.exists(CLI_OUT) and \
            all(os.path.getmtime(d) <= os.path.getmtime(CLI_OUT) for d in CLI_DEPS + [lib]):
        return CLI_OUT
    os.makedirs(BIN_DIR, exist_ok=True)
    cxx = os.environ.get("CXX", "g++")
    cmd = [cxx, "-O2", "-std=c++17", "-Wall", "-o", CLI_OUT + ".tmp",
           os.path.join(CSRC, "oic_main.cpp"), "-L" + OUT_DIR, "-lcanu_ovl",
           "-Wl,-rpath,$ORIGIN/../lib", "-Wl,--allow-shlib-undefined"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True, cwd=CSRC)
    os.replace(CLI_OUT + ".tmp", CLI_OUT)
    return CLI_OUT


MHAP_CLI_OUT = os.path.join(BIN_DIR, "mhap")


def build_mhap_cli(force: bool = False, verbose: bool = True) -> str:
    """canu_amd/bin/mhap: the MHAP command line canu's mhap.sh / precompute.sh run (host
    C++ over libcanu_mhap.so, found next to it through the rpath; zlib for -f .gz)."""
    lib = build_mhap(verbose=verbose)
    src = os.path.join(CSRC, "mhap_main.cpp")
    deps = [src, lib, os.path.join(HERE, "..", "include", "canu_mhap.h")]
    if not force and os.path.exists(MHAP_CLI_OUT) and \
            all(os.path.getmtime(d) <= os.path.getmtime(MHAP_CLI_OUT) for d in deps):
        return MHAP_CLI_OUT
    os.makedirs(BIN_DIR, exist_ok=True)
    cxx = os.environ.get("CXX", "g++")
    cmd = [cxx, "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(HERE, "..", "include"),
           "-o", MHAP_CLI_OUT + ".tmp", src, "-L" + OUT_DIR, "-lcanu_mhap", "-lz",
           "-Wl,-rpath,$ORIGIN/../lib", "-Wl,--allow-shlib-undefined"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True, cwd=CSRC)
    os.replace(MHAP_CLI_OUT + ".tmp", MHAP_CLI_OUT)
    return MHAP_CLI_OUT


MERYL_OUT = os.path.join(OUT_DIR, "libcanu_meryl.so")
MERYL_DEPS = [os.path.join(CSRC, "meryl.hip"), os.path.join(CSRC, "meryl_host.h"),
              os.path.join(HERE, "..", "include", "canu_meryl.h")]
MERYL_CLI_OUT = os.path.join(BIN_DIR, "meryl")
EMT_CLI_OUT = os.path.join(BIN_DIR, "estimate-mer-threshold")


def _stale(out: str, deps: list) -> bool:
    return not os.path.exists(out) or \
        any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps)


def build_meryl(force: bool = False, verbose: bool = True) -> str:
    """canu_amd/lib/libcanu_meryl.so: the k-mer count (meryl's frequent-mer step)."""
    if not force and not _stale(MERYL_OUT, MERYL_DEPS):
        return MERYL_OUT
    os.makedirs(OUT_DIR, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, *HIPCC_FLAGS, "-o", MERYL_OUT + ".tmp", os.path.join(CSRC, "meryl.hip")]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True, cwd=CSRC)
    os.replace(MERYL_OUT + ".tmp", MERYL_OUT)
    return MERYL_OUT


def build_meryl_cli(force: bool = False, verbose: bool = True) -> str:
    """canu_amd/bin/meryl: the three meryl command lines canu's 0-mercounts stage runs (host
    C++ over libcanu_meryl.so, found next to it through the rpath)."""
    lib = build_meryl(verbose=verbose)
    src = os.path.join(CSRC, "meryl_main.cpp")
    deps = [src, lib, os.path.join(CSRC, "gkp_store.h"), *MERYL_DEPS[1:]]
    if not force and not _stale(MERYL_CLI_OUT, deps):
        return MERYL_CLI_OUT
    os.makedirs(BIN_DIR, exist_ok=True)
    cxx = os.environ.get("CXX", "g++")
    cmd = [cxx, "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(HERE, "..", "include"),
           "-o", MERYL_CLI_OUT + ".tmp", src, "-L" + OUT_DIR, "-lcanu_meryl",
           "-Wl,-rpath,$ORIGIN/../lib", "-Wl,--allow-shlib-undefined"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True, cwd=CSRC)
    os.replace(MERYL_CLI_OUT + ".tmp", MERYL_CLI_OUT)
    return MERYL_CLI_OUT


def build_emt_cli(force: bool = False, verbose: bool = True) -> str:
    """canu_amd/bin/estimate-mer-threshold: host only, no library."""
    src = os.path.join(CSRC, "emt_main.cpp")
    if not force and not _stale(EMT_CLI_OUT, [src]):
        return EMT_CLI_OUT
    os.makedirs(BIN_DIR, exist_ok=True)
    cxx = os.environ.get("CXX", "g++")
    cmd = [cxx, "-O2", "-std=c++17", "-Wall", "-o", EMT_CLI_OUT + ".tmp", src]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True, cwd=CSRC)
    os.replace(EMT_CLI_OUT + ".tmp", EMT_CLI_OUT)
    return EMT_CLI_OUT


PAIR_OUT = os.path.join(OUT_DIR, "libcanu_pair.so")
PAIR_DEPS = [os.path.join(CSRC, "pair.hip"), os.path.join(HERE, "..", "include", "canu_pair.h"),
             os.path.join(HERE, "..", "include", "canu_ovl.h")]
PAIR_CLI_OUT = os.path.join(BIN_DIR, "overlapPair")


def build_pair(force: bool = False, verbose: bool = True) -> str:
    """canu_amd/lib/libcanu_pair.so: overlapPair, the exact realignment of MHAP overlaps."""
    if not force and not _stale(PAIR_OUT, PAIR_DEPS):
        return PAIR_OUT
    os.makedirs(OUT_DIR, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, *HIPCC_FLAGS, "-o", PAIR_OUT + ".tmp", os.path.join(CSRC, "pair.hip")]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True, cwd=CSRC)
    os.replace(PAIR_OUT + ".tmp", PAIR_OUT)
    return PAIR_OUT


def build_pair_cli(force: bool = False, verbose: bool = True) -> str:
    """canu_amd/bin/overlapPair: the command line canu's mhap.sh runs after mhapConvert (host
    C++ over libcanu_pair.so, found next to it through the rpath)."""
    lib = build_pair(verbose=verbose)
    src = os.path.join(CSRC, "pair_main.cpp")
    deps = [src, lib, os.path.join(CSRC, "gkp_store.h"), os.path.join(CSRC, "ovl_ovb.h"),
            os.path.join(CSRC, "ovb_reader.h"), *PAIR_DEPS[1:]]
    if not force and not _stale(PAIR_CLI_OUT, deps):
        return PAIR_CLI_OUT
    os.makedirs(BIN_DIR, exist_ok=True)
    cxx = os.environ.get("CXX", "g++")
    cmd = [cxx, "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(HERE, "..", "include"),
           "-o", PAIR_CLI_OUT + ".tmp", src, "-L" + OUT_DIR, "-lcanu_pair",
           "-Wl,-rpath,$ORIGIN/../lib", "-Wl,--allow-shlib-undefined"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True, cwd=CSRC)
    os.replace(PAIR_CLI_OUT + ".tmp", PAIR_CLI_OUT)
    return PAIR_CLI_OUT


FE_OUT = os.path.join(OUT_DIR, "libcanu_fe.so")
FE_DEPS = [os.path.join(CSRC, "fe.hip"), os.path.join(HERE, "..", "include", "canu_fe.h"),
           os.path.join(HERE, "..", "include", "canu_ovl.h")]


def build_fe(force: bool = False, verbose: bool = True) -> str:
    """canu_amd/lib/libcanu_fe.so: findErrors, read error detection from the overlaps."""
    if not force and not _stale(FE_OUT, FE_DEPS):
        return FE_OUT
    os.makedirs(OUT_DIR, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, *HIPCC_FLAGS, "-o", FE_OUT + ".tmp", os.path.join(CSRC, "fe.hip")]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True, cwd=CSRC)
    os.replace(FE_OUT + ".tmp", FE_OUT)
    return FE_OUT


FE_CLI_OUT = os.path.join(BIN_DIR, "findErrors")


def build_fe_cli(force: bool = False, verbose: bool = True) -> str:
    """canu_amd/bin/findErrors: the command line canu's red.sh runs (host C++ over
    libcanu_fe.so, found next to it through the rpath)."""
    lib = build_fe(verbose=verbose)
    src = os.path.join(CSRC, "fe_main.cpp")
    deps = [src, lib, os.path.join(CSRC, "gkp_store.h"), os.path.join(CSRC, "ovs_reader.h"),
            *FE_DEPS[1:]]
    if not force and not _stale(FE_CLI_OUT, deps):
        return FE_CLI_OUT
    os.makedirs(BIN_DIR, exist_ok=True)
    cxx = os.environ.get("CXX", "g++")
    cmd = [cxx, "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(HERE, "..", "include"),
           "-o", FE_CLI_OUT + ".tmp", src, "-L" + OUT_DIR, "-lcanu_fe",
           "-Wl,-rpath,$ORIGIN/../lib", "-Wl,--allow-shlib-undefined"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True, cwd=CSRC)
    os.replace(FE_CLI_OUT + ".tmp", FE_CLI_OUT)
    return FE_CLI_OUT


CO_OUT = os.path.join(OUT_DIR, "libcanu_co.so")
CO_DEPS = [os.path.join(CSRC, "co.hip"), os.path.join(HERE, "..", "include", "canu_co.h"),
           os.path.join(HERE, "..", "include", "canu_fe.h"),
           os.path.join(HERE, "..", "include", "canu_ovl.h")]
CO_CLI_OUT = os.path.join(BIN_DIR, "correctOverlaps")


def build_co(force: bool = False, verbose: bool = True) -> str:
    """canu_amd/lib/libcanu_co.so: correctOverlaps, overlap error rates from corrected reads."""
    if not force and not _stale(CO_OUT, CO_DEPS):
        return CO_OUT
    os.makedirs(OUT_DIR, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, *HIPCC_FLAGS, "-o", CO_OUT + ".tmp", os.path.join(CSRC, "co.hip")]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True, cwd=CSRC)
    os.replace(CO_OUT + ".tmp", CO_OUT)
    return CO_OUT


def build_co_cli(force: bool = False, verbose: bool = True) -> str:
    """canu_amd/bin/correctOverlaps: the command line canu's oea.sh runs (host C++ over
    libcanu_co.so, found next to it through the rpath)."""
    lib = build_co(verbose=verbose)
    src = os.path.join(CSRC, "co_main.cpp")
    deps = [src, lib, os.path.join(CSRC, "gkp_store.h"), os.path.join(CSRC, "ovs_reader.h"),
            os.path.join(CSRC, "co_files.h"), *CO_DEPS[1:]]
    if not force and not _stale(CO_CLI_OUT, deps):
        return CO_CLI_OUT
    os.makedirs(BIN_DIR, exist_ok=True)
    cxx = os.environ.get("CXX", "g++")
    cmd = [cxx, "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(HERE, "..", "include"),
           "-o", CO_CLI_OUT + ".tmp", src, "-L" + OUT_DIR, "-lcanu_co",
           "-Wl,-rpath,$ORIGIN/../lib", "-Wl,--allow-shlib-undefined"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True, cwd=CSRC)
    os.replace(CO_CLI_OUT + ".tmp", CO_CLI_OUT)
    return CO_CLI_OUT


FS_OUT = os.path.join(OUT_DIR, "libcanu_fs.so")
FS_DEPS = [os.path.join(CSRC, "fs.hip"), os.path.join(CSRC, "fs_fasta.h"),
           os.path.join(HERE, "..", "include", "canu_fs.h")]
FS_CLI_OUT = os.path.join(BIN_DIR, "falconsense")


def build_fs(force: bool = False, verbose: bool = True) -> str:
    """canu_amd/lib/libcanu_fs.so: falconsense, corrected reads from correction layouts."""
    if not force and not _stale(FS_OUT, FS_DEPS):
        return FS_OUT
    os.makedirs(OUT_DIR, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, *HIPCC_FLAGS, "-o", FS_OUT + ".tmp", os.path.join(CSRC, "fs.hip")]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True, cwd=CSRC)
    os.replace(FS_OUT + ".tmp", FS_OUT)
    return FS_OUT


def build_fs_cli(force: bool = False, verbose: bool = True) -> str:
    """canu_amd/bin/falconsense: the command line canu's correctReads.sh runs (host C++ over
    libcanu_fs.so, found next to it through the rpath)."""
    lib = build_fs(verbose=verbose)
    src = os.path.join(CSRC, "fs_main.cpp")
    deps = [src, lib, os.path.join(CSRC, "gkp_store.h"), os.path.join(CSRC, "tgs_reader.h"),
            *FS_DEPS[1:]]
    if not force and not _stale(FS_CLI_OUT, deps):
        return FS_CLI_OUT
    os.makedirs(BIN_DIR, exist_ok=True)
    cxx = os.environ.get("CXX", "g++")
    cmd = [cxx, "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(HERE, "..", "include"),
           "-o", FS_CLI_OUT + ".tmp", src, "-L" + OUT_DIR, "-lcanu_fs",
           "-Wl,-rpath,$ORIGIN/../lib", "-Wl,--allow-shlib-undefined"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True, cwd=CSRC)
    os.replace(FS_CLI_OUT + ".tmp", FS_CLI_OUT)
    return FS_CLI_OUT


def build(force: bool = False, verbose: bool = True, profile: bool = False) -> str:
    """profile=True builds the instrumented variant (in-kernel cycle stamps, OVL_DEBUG=1
    prints them) as libcanu_ovl_prof.so; load it with CANU_OVL_LIB."""
    out = PROF_OUT if profile else OUT
    if not force and not profile and not needs_build():
        return out
    os.makedirs(OUT_DIR, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    extra = ["-DOVL_PROFILE"] if profile else []
    cmd = [hipcc, *HIPCC_FLAGS, *extra, "-o", out + ".tmp", os.path.join(CSRC, "ovl_api.hip")]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True, cwd=CSRC)
    os.replace(out + ".tmp", out)
    return out


if __name__ == "__main__":
    build(force="--force" in sys.argv, profile="--profile" in sys.argv)
    if "--profile" not in sys.argv:
        build_mhap(force="--force" in sys.argv)
        build_cli(force="--force" in sys.argv)
        build_meryl(force="--force" in sys.argv)
        build_meryl_cli(force="--force" in sys.argv)
        build_emt_cli(force="--force" in sys.argv)
        build_pair(force="--force" in sys.argv)
        build_pair_cli(force="--force" in sys.argv)
        build_fe(force="--force" in sys.argv)
        build_fe_cli(force="--force" in sys.argv)
        build_co(force="--force" in sys.argv)
        build_co_cli(force="--force" in sys.argv)
        build_fs(force="--force" in sys.argv)
        build_fs_cli(force="--force" in sys.argv)
