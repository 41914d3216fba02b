"""Is the device code of two sets of host objects the same, kernel by kernel?
    python tools/kernels_equal.py A.o B.o                  two objects
    python tools/kernels_equal.py a1.o,a2.o,... b1.o,...   two comma-separated lists
    python tools/kernels_equal.py DIR_A DIR_B              every *.o directly in each directory

Each side is the union of the kernels of its objects, keyed by symbol, so kernels may move between objects (a kernel that
two objects of one side carry in different versions is reported; the profiling build's *_ablate.o objects are a set of
their own, compared with the other side's).  Point it at csrc/*.o, not at libALS.so: the linked library carries one
offload bundle per translation unit back to back, and one --unbundle may see only the first.  Per
kernel it compares the instructions (llvm-objdump, with branch-target labels, trailing comments and the PC-relative
literal after each s_getpc_b64 normalised: that offset to a global such as g_wave_zeros moves when the kernel order
changes) and the register / LDS / scratch / kernarg metadata (llvm-readelf --notes).  Kernels present on one side only are
reported.  Prints SAME or DIFFERENT (exit status 0 / 1).  No GPU needed."""
import os, re, subprocess, sys, tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
META = ("agpr_count", "sgpr_count", "vgpr_count", "sgpr_spill_count", "vgpr_spill_count", "group_segment_fixed_size",
        "private_segment_fixed_size", "kernarg_segment_size")


def code_object(obj, tmp):
    fatbin, co = os.path.join(tmp, "x.fatbin"), os.path.join(tmp, "x.co")
    subprocess.run([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fatbin], check=True)
    if os.path.getsize(fatbin) == 0:  # a host-only object
        return None
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fatbin}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True, capture_output=True)
    return co


def kernels(obj):
    """{symbol: (normalised instructions, metadata)} of every kernel in obj's gfx950 code object."""
    with tempfile.TemporaryDirectory() as tmp:
        co = code_object(obj, tmp)
        if co is None:
            return {}
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co],
                             check=True, capture_output=True, text=True).stdout
        syms = subprocess.run([f"{LLVM}/llvm-readelf", "-s", "--wide", co], check=True, capture_output=True, text=True).stdout
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    # end address of every function: the padding words behind a kernel (alignment of the next one) are not its code
    end = {m.group(3): int(m.group(1), 16) + int(m.group(2), 0)  # (readelf prints large sizes in hex)
           for m in re.finditer(r"^\s*\d+:\s+([0-9a-f]+)\s+(0x[0-9a-f]+|\d+)\s+FUNC\s+\S+\s+\S+\s+\S+\s+(\S+)$", syms, re.M)}
    code = {}
    name = None
    after_getpc = False
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line.strip())
        if m:
            name = m.group(1)
            code[name] = []
            after_getpc = False
            continue
        ins, _, comment = line.partition("//")
        ins = ins.strip()
        if name is None or not ins or ins == "..." or re.match(r"^\S+:$", ins):  # "...": zero padding
            continue
        addr = re.match(r"\s*([0-9A-Fa-f]+):", comment)
        if addr and name in end and int(addr.group(1), 16) >= end[name]:
            continue
        ins = re.sub(r"\s+<[^>]*>", "", ins)  # branch targets: <symbol+offset>
        if after_getpc and ins.startswith("s_add_u32"):
            ins = re.sub(r",\s*\S+$", ", <pcrel>", ins)
        after_getpc = ins.startswith("s_getpc_b64")
        code[name].append(ins)
    meta = {}
    for blk in re.split(r"\n\s+- \.agpr_count", notes)[1:]:
        blk = ".agpr_count" + blk
        sym = re.search(r"\.symbol:\s+(\S+)", blk)
        kname = sym.group(1)[:-3] if sym and sym.group(1).endswith(".kd") else re.search(r"\.name:\s+(\S+)", blk).group(1)
        meta[kname] = tuple((k, (re.search(r"\." + k + r":\s+(\S+)", blk) or [None, "?"])[1]) for k in META)
    return {k: (code.get(k), meta[k]) for k in meta}


def objects(arg):
    if os.path.isdir(arg):
        return sorted(os.path.join(arg, f) for f in os.listdir(arg) if f.endswith(".o"))
    return arg.split(",")


def side(arg, diffs):
    """{symbol: (instructions, metadata)} over every object of one side."""
    out = {}
    for obj in objects(arg):
        # the profiling build's objects (*_ablate.o) carry kernels of the product's names compiled with other switches
        tag = " [ablate]" if os.path.basename(obj).endswith("_ablate.o") else ""
        for k, v in kernels(obj).items():
            k += tag
            if k in out and out[k] != v:
                diffs.append(f"two versions of {k} in {arg}")
            out[k] = v
    return out


def main():
    a, b = sys.argv[1], sys.argv[2]
    diffs = []
    ka, kb = side(a, diffs), side(b, diffs)
    diffs += [f"only in {a}: {k}" for k in sorted(set(ka) - set(kb))] + [f"only in {b}: {k}" for k in sorted(set(kb) - set(ka))]
    for k in sorted(set(ka) & set(kb)):
        (ca, ma), (cb, mb) = ka[k], kb[k]
        if ma != mb:
            diffs.append(f"metadata of {k}: {dict(ma)} vs {dict(mb)}")
        if ca != cb:
            n = next((i for i, (x, y) in enumerate(zip(ca or [], cb or [])) if x != y), min(len(ca or []), len(cb or [])))
            diffs.append(f"instructions of {k}: first difference at {n}")
    for d in diffs:
        print(d)
    print(f"{'SAME' if not diffs else 'DIFFERENT'} ({len(ka)} / {len(kb)} kernels)")
    return 1 if diffs else 0


if __name__ == "__main__":
    sys.exit(main())
