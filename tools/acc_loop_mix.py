#!/usr/bin/env python3
"""Instruction mix of the bucket-accumulation hot loop, from the compiler's assembly.  No GPU needed.

Compiles csrc/zkt_msm.hip to gfx950 assembly with exactly the flags of the Makefile's zkt_msm.o rule (the G1 object; the command line is
taken from `make -n`, so the two cannot drift apart), finds k_accumulate of the G1 field, and prints for every basic block above --min-block
instructions its size, its VALU mix (ordinary v_* mnemonics) and its s_nop count, then the kernel's register, scratch and occupancy
figures from the code object's metadata.  The steady-state iteration of the accumulate loop is the sum of those blocks without the doubling exits, which are
told by their multiply-add count (about 2,333 in one block; the mixed addition's 8 products, 2 squarings and 9 reductions are about 3,550 over its blocks); its totals are printed last.
With the object on 13 x 30-bit limbs (the Makefile's FQ30FLAGS, part of the command line taken from `make -n`) the kernel is k_accumulate<PrimeOps<Fq30C>>, a doubling exit
holds about 2,021 multiply-adds and the mixed addition about 3,090.  `make -n` is run with this process's environment, so FQ30FLAGS= in the environment gives the 14 x 28 object.

usage: tools/acc_loop_mix.py [--min-block 300] [--kernel k_accumulate] [--keep out.s | --asm in.s] [extra compiler flags ...]
"""
import argparse, collections, os, re, shlex, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "zk-toolkit_amd")


def compile_to_asm(out_s, extra):
    with tempfile.TemporaryDirectory() as obj:
        plan = subprocess.run(["make", "-n", "-B", "-C", PKG, "OBJ=" + obj, obj + "/zkt_msm.o"], capture_output=True, text=True, check=True).stdout
    line = [l for l in plan.splitlines() if "zkt_msm.hip" in l and " -c " in l]
    assert len(line) == 1, plan
    cmd = shlex.split(line[0])
    cmd = cmd[:cmd.index("-o")] + cmd[cmd.index("-o") + 2:]
    cmd[cmd.index("-c")] = "-S"
    cmd += ["--cuda-device-only", "-o", out_s] + extra
    subprocess.run(cmd, cwd=PKG, check=True)
    return " ".join(cmd)


def kernel_body(text, want):
    """(mangled name, lines) of the one kernel whose name holds `want`, instantiated for Fq"""
    m = [n for n in re.findall(r"^(_Z\w+):", text, re.M) if want in n and ("3FqC" in n or "5Fq30C" in n)]      # the G1 object's field: 14 x 28 or 13 x 30 limbs
    assert len(m) == 1, m
    name = m[0]
    body = text[text.index("\n" + name + ":"):text.index(".Lfunc_end", text.index("\n" + name + ":"))]
    return name, body.splitlines()[2:]


def blocks(lines):
    cur, out = "entry", collections.OrderedDict()
    out[cur] = []
    for l in lines:
        s = l.split(";")[0].strip()
        if not s: continue
        if re.match(r"^\.?\w+:$", s): cur = s[:-1]; out[cur] = []; continue
        if s.startswith("."): continue
        out[cur].append(s.split()[0])
    return out


def meta(text, name):
    recs = re.split(r"\n  - ", text[text.index("amdhsa.kernels"):])
    rec = [r for r in recs if re.search(r"\.name:\s+" + re.escape(name) + r"\s", r)][0]
    get = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", rec).group(1))
    tail = text[text.index(".Lfunc_end", text.index("\n" + name + ":")):]
    occ = re.search(r"; Occupancy:\s+(\d+)", tail)
    return {"vgpr": get("vgpr_count"), "agpr": get("agpr_count"), "vgpr_spill": get("vgpr_spill_count"), "sgpr": get("sgpr_count"),
            "scratch_bytes": get("private_segment_fixed_size"), "occupancy": int(occ.group(1)) if occ else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-block", type=int, default=300)
    ap.add_argument("--kernel", default="k_accumulate")
    ap.add_argument("--keep", help="write the assembly here")
    ap.add_argument("--asm", help="read this assembly instead of compiling")
    args, extra = ap.parse_known_args()
    if args.asm:
        cmd, text = "(read from " + os.path.basename(args.asm) + ")", open(args.asm).read()
    else:
        with tempfile.TemporaryDirectory() as td:
            out_s = args.keep or os.path.join(td, "zkt_msm.s")
            cmd = compile_to_asm(os.path.abspath(out_s), extra)
            text = open(out_s).read()
    name, lines = kernel_body(text, args.kernel)
    loop = collections.Counter()
    dbl_exit = 2021 if "5Fq30C" in name else 2333      # multiply-adds of a doubling-exit block: 13 x 30 limbs (338 per product), 14 x 28 (392)
    print("# " + re.sub(r"\S*/(?=zkt_msm\.s)", "", cmd.replace(ROOT + "/", "")))
    print("kernel %s" % name)
    for label, ins in blocks(lines).items():
        if len(ins) <= args.min_block: continue
        mix = collections.Counter(i for i in ins if i.startswith("v_"))
        print("block %s: %d instructions, %d VALU, %d s_nop, %d s_waitcnt" % (label, len(ins), sum(mix.values()), sum(1 for i in ins if i == "s_nop"), sum(1 for i in ins if i == "s_waitcnt")))
        print("   " + "  ".join("%s %d" % (k.replace("_e32", "").replace("_e64", ""), v) for k, v in mix.most_common() if v >= 8) + "  (others %d)" % sum(v for v in mix.values() if v < 8))
        # the mixed addition: every big block but the doubling exits, which hold two squarings more and two products fewer and so about 2,333 multiply-adds
        if abs(mix["v_mad_u64_u32"] - dbl_exit) > 20:
            loop.update(ins); loop["blocks"] += 1
    print("steady-state iteration (the %d blocks above that are not doubling exits): %d instructions, %d v_mad_u64_u32, %d v_lshl_add_u64, %d s_nop" %
          (loop.pop("blocks", 0), sum(loop.values()), loop["v_mad_u64_u32"], loop["v_lshl_add_u64"], loop["s_nop"]))
    m = meta(text, name)
    print("vgpr %(vgpr)d  agpr %(agpr)d  vgpr_spill %(vgpr_spill)d  sgpr %(sgpr)d  scratch %(scratch_bytes)d B  occupancy %(occupancy)s" % m)


if __name__ == "__main__":
    main()
