"""Compare the gfx950 device code of two builds of one library, kernel by kernel.

usage: python tools/isa_compare.py parent.so new.so > profiles/NAME.txt

Takes the gfx950 code object out of each library (.hip_fatbin section, clang-offload-bundler
--unbundle) and compares, per kernel symbol, the metadata of llvm-readelf --notes (registers,
spills, LDS, private segment, kernarg size, workgroup size, wave size) and the instructions of
llvm-objdump -d without addresses, comments, the padding between functions and the distance
in a PC-relative address (it moves with the kernel's place in the file).  Exit status 1
when the kernel sets differ or a kernel of the project (not rocprim / hipcub) differs.
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
META = [".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
        ".group_segment_fixed_size", ".private_segment_fixed_size", ".kernarg_segment_size",
        ".max_flat_workgroup_size", ".wavefront_size"]


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def code_object(lib, tmp):
    fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "gfx950.co")
    run(f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", lib, os.devnull)
    run(f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}",
        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}")
    return co


def kernels(lib):
    """{demangled kernel name: (metadata tuple, [instructions], [PC-relative literals])}"""
    with tempfile.TemporaryDirectory() as tmp:
        co = code_object(lib, tmp)
        notes = run(f"{LLVM}/llvm-readelf", "--notes", co)
        dis = run(f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co)
    meta = {}
    for block in re.split(r"\n\s+- \.agpr_count:", "\n" + notes)[1:]:
        block = "      .agpr_count:" + block
        sym = re.search(r"\.symbol:\s+'?([^'\s]+?)\.kd'?\s", block).group(1)
        meta[sym] = tuple(int(m.group(1)) if (m := re.search(re.escape(f) + r":\s+(\d+)", block))
                          else 0 for f in META)
    code, cur, pcrel, sym_now = {}, None, {}, None
    for line in dis.splitlines():
        m = re.match(r"[0-9a-f]+ <(.+)>:$", line)
        if m:
            sym_now = m.group(1)
            cur = code.setdefault(sym_now, []) if sym_now in meta else None
        elif cur is not None and line.strip():
            ins = re.sub(r"\s*//.*$", "", line).strip()
            ins = re.sub(r"^[0-9a-f]+:\s+", "", ins)
            if ins and ins != "..." and not ins.startswith("s_code_end"):   # "...": zero padding
                # the low half of a PC-relative address (s_getpc_b64, then s_add_u32 with the
                # distance to a symbol) moves with the kernel's place in the file
                if cur and cur[-1].startswith("s_getpc_b64") and ins.startswith("s_add_u32"):
                    pcrel.setdefault(sym_now, []).append(ins.rsplit(" ", 1)[-1])
                    ins = re.sub(r"0x[0-9a-f]+$", "<pc-relative>", ins)
                cur.append(ins)
    for c in code.values():                          # the padding behind a function's end
        while c and c[-1].startswith("s_nop"):
            c.pop()
    names = subprocess.run(["c++filt"], input="\n".join(meta), check=True, capture_output=True,
                           text=True).stdout.splitlines()
    return {n: (meta[s], code.get(s, []), pcrel.get(s, [])) for s, n in zip(meta, names)}


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    print(f"kernel symbols: parent {len(a)}, new {len(b)}; only in parent: "
          f"{', '.join(only_a) or 'none'}; only in new: {', '.join(only_b) or 'none'}\n")
    print(f"{'kernel (both builds unless marked)':64}  VGPR  SGPR v-spill s-spill   LDS B  private"
          "   insts  metadata / code")
    lib_equal, differ, bad = 0, 0, bool(only_a or only_b)
    lit_n = lit_same = 0
    for n in sorted(set(a) & set(b)):
        (ma, ca, la), (mb, cb, lb) = a[n], b[n]
        lit_n += len(la)
        lit_same += sum(x == y for x, y in zip(la, lb))
        ours = not n.startswith(("rocprim::", "hipcub::", "void rocprim::", "void hipcub::"))
        same = ma == mb and ca == cb
        differ += not same
        bad |= ours and not same
        if not ours and same:
            lib_equal += 1
            continue
        print(f"{n[:64]:64} {ma[0]:5} {ma[2]:5} {ma[3]:7} {ma[4]:7} {ma[5]:7} {ma[6]:8} {len(ca):7}  "
              f"{'equal' if ma == mb else 'DIFFERENT'} / {'equal' if ca == cb else 'DIFFERENT'}")
        if ca != cb and len(ca) == len(cb):
            for x, y in zip(ca, cb):
                if x != y:
                    print(f"    {x}   ->   {y}")
    print(f"\nlibrary kernels (rocprim / hipcub instantiations) not listed, all equal in metadata "
          f"and code: {lib_equal}\nkernels that differ: {differ}\nPC-relative literals (masked in the "
          f"comparison above): {lit_n}, equal as they stand in both builds: {lit_same}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
