#!/usr/bin/env python3
"""Generate zk-toolkit_amd/csrc/zkt_constants.h: Montgomery constants (32-bit limbs)
for the four prime fields of the hot path and the curve constants derived from them.

Moduli / generators are the reference's (paths relative to /root/reference):
  q, r        src/building_block/curves/bls12_381/params.rs:9,14
  G1, G2 gen  src/building_block/curves/bls12_381/g1_point.rs:41,44; g2_point.rs:37-43
  secp256k1   src/building_block/curves/secp256k1/affine_point.rs:30-47
"""
import os

Q = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
SP = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEFFFFFC2F
SN = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
X_ABS = 0xd201000000010000   # |x|, BLS parameter x = -X_ABS (r = x^4 - x^2 + 1)
assert R == X_ABS**4 - X_ABS**2 + 1


def limbs(x, n):
    return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def arr(x, n):
    return "{" + ",".join("0x%08xu" % v for v in limbs(x, n)) + "}"


def limbs_w(x, n, w):
    return [(x >> (w * i)) & ((1 << w) - 1) for i in range(n)]


def arr_w(v):
    return "{" + ",".join("0x%08xu" % t for t in v) + "}"


def field(name, p, n, doc, w=32):
    """w = 32: n x 32-bit limbs, canonical Montgomery residues, carry-chain add/sub (Fr, secp256k1 fields).
       w = 28: n x 28-bit limbs, lazy residues < 4p, R = 2^(28n): the multiply needs no carry chain (Fq, the hot field).
       w = 30: the same lazy form on n x 30-bit limbs (Fq in the G1 MSM object: 13 limbs instead of 14).  A full column of a product scan no longer
               fits 64 bits; split_masks() below derives, from exact worst-case bounds, where a column's running sum must hand its carry over."""
    Rm = (1 << (w * n)) % p
    inv = (-pow(p, -1, 1 << w)) % (1 << w)
    abi_n = (p.bit_length() + 31) // 32
    s = []
    s.append(f"// {doc}")
    s.append(f"struct {name} {{")
    s.append(f"  static constexpr int N = {n};        // internal limbs")
    s.append(f"  static constexpr int W = {w};        // bits per limb")
    s.append(f"  static constexpr int ABI_N = {abi_n};    // 32-bit words of a canonical residue at the boundary")
    s.append(f"  static constexpr uint32_t INV = 0x{inv:08x}u;   // -p^-1 mod 2^W")
    tabs = [("mod", limbs_w(p, n, w)), ("one", limbs_w(Rm, n, w)), ("r2", limbs_w(Rm * Rm % p, n, w))]
    if w == 32:
        tabs += [("r3", limbs_w(Rm * Rm * Rm % p, n, w))]
    for fn, val in tabs:
        s.append(f"  ZKT_HD static constexpr uint32_t {fn}(int i) {{ constexpr uint32_t t[{n}] = {arr_w(val)}; return t[i]; }}")
    s.append(f"  ZKT_HD static constexpr uint32_t mod32(int i) {{ constexpr uint32_t t[{abi_n}] = {arr_w(limbs_w(p, abi_n, 32))}; return t[i]; }}")
    s.append(f"  ZKT_HD static constexpr uint32_t pm2(int i) {{ constexpr uint32_t t[{abi_n}] = {arr_w(limbs_w(p - 2, abi_n, 32))}; return t[i]; }}   // p-2, 32-bit words")
    if w in (28, 30):
        k8 = limbs_w(8 * p, n, w)
        subk = [k8[0] + (1 << w)] + [k8[i] + (1 << w) - 1 for i in range(1, n - 1)] + [k8[n - 1] - 1]
        assert sum(v << (w * i) for i, v in enumerate(subk)) == 8 * p and all(v >= (1 << w) - 1 for v in subk[:-1])
        assert subk[-1] >= (4 * p) >> (w * (n - 1))          # top limb covers any subtrahend < 4p
        top = p >> (w * (n - 1))
        s.append(f"  ZKT_HD static constexpr uint32_t subk(int i) {{ constexpr uint32_t t[{n}] = {arr_w(subk)}; return t[i]; }}   // 8p with borrow-safe limbs")
        k16 = limbs_w(16 * p, n, w)
        # every limb must cover b + 2c <= 3 (2^w - 1): lend 4 units of the next limb where a u32 has the room (w = 28), 3 where it has not (w = 30)
        lend = 4 if w == 28 else 3
        subk3 = [k16[0] + lend * (1 << w)] + [k16[i] + lend * (1 << w) - lend for i in range(1, n - 1)] + [k16[n - 1] - lend]
        assert sum(v << (w * i) for i, v in enumerate(subk3)) == 16 * p and all(v >= 3 * ((1 << w) - 1) for v in subk3[:-1])
        assert subk3[-1] >= 3 * ((4 * p) >> (w * (n - 1))) + 3
        if w == 28:
            assert max(subk3) + (1 << w) < (1 << 31)
        else:
            # w = 30: a + subk - b (+ the reduction's carry < 2^6) fits a u32; subk3 - b - 2c fits a u32 on its own and meets a in the 64-bit sum of fp_lazy_reduce2
            assert max(subk) + (1 << w) + 64 < (1 << 32) and max(subk3) < (1 << 32)
        s.append(f"  ZKT_HD static constexpr uint32_t subk3(int i) {{ constexpr uint32_t t[{n}] = {arr_w(subk3)}; return t[i]; }}   // 16p, every limb covers b + 2c for b, c < 4p")
        s.append(f"  ZKT_HD static constexpr uint32_t comp(int i) {{ constexpr uint32_t t[{n}] = {arr_w(limbs_w((1 << (w * n)) - p, n, w))}; return t[i]; }}   // 2^(WN) - p")
        s.append(f"  static constexpr uint32_t QEST_M = {(1 << 32) // (top + 1)}u;   // floor(2^32 / (floor(p / 2^(W(N-1))) + 1))")
        body = "{" + ",".join(arr_w(limbs_w(j * p, n, w)) for j in range(4)) + "}"
        s.append(f"  ZKT_HD static constexpr uint32_t kp(int j, int i) {{ constexpr uint32_t t[4][{n}] = {body}; return t[j][i]; }}   // j*p, j<4")
    if w == 30:
        masks, carry = split_masks(limbs_w(p, n, w), subk, n, w)
        for kind in ("mul", "sqr", "mul2"):
            vals = "{" + ",".join("0x%xull" % v for v in masks[kind]) + "}"
            cols = [k for k, v in enumerate(masks[kind]) if v]
            s.append(f"  // columns {cols}; the carry out of a column stays below 2^{max(carry[kind]).bit_length()}")
            s.append(f"  ZKT_HD static constexpr uint64_t split_{kind}(int k) {{ constexpr uint64_t t[{2 * n}] = {vals}; return t[k]; }}")
    s.append("};")
    return "\n".join(s)


def scan_terms(kind, k, pl, subk, n, w):
    """Worst-case value of every multiply-add of column k of a product scan, in the order fp.h issues them (limbs < 2^w on both sides unless said otherwise):
       mul   a_i b_(k-i), then m_j p_(k-j) with the exact limbs of p
       sqr   (2 a_i) a_(k-i) for 2i < k, a_(k/2)^2, then the reduction
       mul2  a_i b_(k-i) and c_i (8p spread - d)_(k-i) alternating, then the reduction"""
    M = (1 << w) - 1
    lo, hi = (0, k) if k < n else (k - n + 1, n - 1)
    t = []
    if kind == "mul":
        t += [M * M for i in range(lo, hi + 1)]
    elif kind == "sqr":
        t += [2 * M * M for i in range(lo, hi + 1) if 2 * i < k] + ([M * M] if k % 2 == 0 else [])
    else:
        for i in range(lo, hi + 1):
            t += [M * M, M * subk[k - i]]
    if k < n:
        t += [M * pl[k - j] for j in range(k)] + [M * pl[0]]
    else:
        t += [M * pl[k - j] for j in range(k - n + 1, n)]
    return t


def split_masks(pl, subk, n, w):
    """Where a column of a 30-bit-limb product scan hands its carry over.  The 64-bit accumulator enters a column with the carry of the one before; bit t of a column's
    mask says: before multiply-add t, move the accumulator's bits above 2^w to a second register and go on from the low w bits.  A split is placed exactly where the
    worst case of the running sum (every operand limb 2^w - 1, the limbs of p and of the 8p spread exact) would reach 2^64, so columns that cannot overflow have mask 0."""
    M = (1 << w) - 1
    masks, carries = {}, {}
    for kind in ("mul", "sqr", "mul2"):
        ms, cs, carry = [], [], 0
        for k in range(2 * n):
            run, hi, mask = carry, 0, 0
            for t, v in enumerate(scan_terms(kind, k, pl, subk, n, w)):
                if run + v >= 1 << 64:
                    mask |= 1 << t; hi += run >> w; run = min(run, M)
                    assert run + v < 1 << 64
                run += v
            carry = (run >> w) + hi
            ms.append(mask); cs.append(carry)
        masks[kind], carries[kind] = ms, cs
    return masks, carries


def mont(x, p, n):
    return x * (1 << (32 * n)) % p


out = []
out.append("// GENERATED by tools/gen_constants.py — do not edit.")
out.append("#pragma once")
out.append("#include <stdint.h>")
out.append("#ifndef ZKT_HD\n#define ZKT_HD __host__ __device__ __forceinline__\n#endif\n// real functions (bounded code size / compile time): big field and tower operations\n#ifndef ZKT_FN\n#define ZKT_FN __host__ __device__ inline __attribute__((noinline))\n#endif")
out.append("namespace zkt {")
out.append(field("FqC", Q, 14, "BLS12-381 base field q (params.rs:9): 14 x 28-bit lazy limbs", w=28))
out.append(field("Fq30C", Q, 13, "BLS12-381 base field q on 13 x 30-bit lazy limbs, R = 2^390: the G1 MSM object (fp.h, W = 30)", w=30))
out.append(field("FrC", R, 8, "BLS12-381 subgroup order r (params.rs:14)"))
out.append(field("SpC", SP, 8, "secp256k1 base field p (secp256k1/affine_point.rs:30-47)"))
out.append(field("SnC", SN, 8, "secp256k1 group order n"))

# final exponentiation pieces (pairing.rs:94-97): (q^12-1)/r = (q^6-1)(q^2+1) * hard,
# hard = (x-1)^2/3 * (x+q) * (x^2+q^2-1) + 1  with x = -X_ABS
x = -X_ABS
hard = ((x - 1) ** 2 // 3) * (x + Q) * (x * x + Q * Q - 1) + 1
assert (x - 1) ** 2 % 3 == 0
assert (Q**12 - 1) // R == (Q**6 - 1) * (Q**2 + 1) * hard and (Q**12 - 1) % R == 0
e1 = (x - 1) ** 2 // 3
out.append(f"static constexpr uint64_t BLS_X_ABS = 0x{X_ABS:x}ull;   // x = -BLS_X_ABS")
out.append(f"static constexpr int E1_BITS = {e1.bit_length()};   // e1 = (x-1)^2/3")
out.append(f"ZKT_HD constexpr uint32_t e1_limb(int i) {{ constexpr uint32_t t[4] = {arr(e1, 4)}; return t[i]; }}")
def _wnaf(k, w):
    d = []
    while k:
        z = 0
        if k & 1:
            z = k % (1 << w)
            if z >= (1 << (w - 1)): z -= (1 << w)
            k -= z
        d.append(z); k //= 2
    return d
e1d = _wnaf(e1, 3)[::-1]                       # most significant first, digits in {0, +-1, +-3}
assert sum(d << (len(e1d) - 1 - i) for i, d in enumerate(e1d)) == e1 and e1d[0] > 0
def _words(bits): return [sum(bits[32 * j + i] << i for i in range(32) if 32 * j + i < len(bits)) for j in range((len(bits) + 31) // 32)]
out.append("// width-3 signed digits of e1 for the hard part of the final exponentiation (inverse = conjugate in the cyclotomic subgroup): 30 products instead of 47")
out.append(f"static constexpr int E1_WNAF_DIGITS = {len(e1d)};")
for nm, bits in (("nz", [1 if d else 0 for d in e1d]), ("neg", [1 if d < 0 else 0 for d in e1d]), ("three", [1 if abs(d) == 3 else 0 for d in e1d])):
    ws = _words(bits)
    out.append(f"ZKT_HD constexpr uint32_t e1_wnaf_{nm}_word(int i) {{ constexpr uint32_t t[{len(ws)}] = {{" + ",".join('0x%08xu' % w for w in ws) + "}; return t[i]; }")
out.append(f"static constexpr int R_BITS = {R.bit_length()};")

# tower constants in Montgomery form (c0 then c1 of each Fq2); validated against generic
# pow(q) by tests/test_fast_model.py::test_frobenius_constants
import sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import fast_model as fm
FQN, FQW = 14, 28
def fq2_arr(c):
    return "{" + ",".join(arr_w(limbs_w(x * (1 << (FQW * FQN)) % Q, FQN, FQW)) for x in c) + "}"
out.append("// xi^-1 = (1+u)^-1 (untwist, g12_point.rs:47-68), Frobenius gamma_i^(k) = xi^(i(q^k-1)/6), i=0..5")
out.append(f"ZKT_HD constexpr uint32_t xi_inv_limb(int c, int i) {{ constexpr uint32_t t[2][{FQN}] = {fq2_arr(fm.XI_INV)}; return t[c][i]; }}")
for k, tab in ((1, fm.FROB1), (2, fm.FROB2)):
    body = "{" + ",".join(fq2_arr(c) for c in tab) + "}"
    out.append(f"ZKT_HD constexpr uint32_t frob{k}_limb(int idx, int c, int i) {{ constexpr uint32_t t[6][2][{FQN}] = {body}; return t[idx][c][i]; }}")
# loop bits of the Miller loop: r-1, MSB first, leading 1 dropped (pairing.rs:58-73), packed LSB-first in u32 words
lb = fm.L_BITS
words = [sum(b << j for j, b in enumerate(lb[i:i + 32])) for i in range(0, len(lb), 32)]
naf = fm.L_NAF
nzw = [sum((1 if naf[32 * j + i] else 0) << i for i in range(32) if 32 * j + i < len(naf)) for j in range((len(naf) + 31) // 32)]
ngw = [sum((1 if naf[32 * j + i] < 0 else 0) << i for i in range(32) if 32 * j + i < len(naf)) for j in range((len(naf) + 31) // 32)]
out.append("// signed digits (NAF, most significant first, leading 1 dropped) of r-1 for the fast Miller loop: 58 non-zero digits instead of 132 one bits;")
out.append("// a chain with subtractions differs from the reference's only by vertical lines, which die in the final exponentiation (oracle/fast_model.py)")
out.append(f"static constexpr int MILLER_NAF_DIGITS = {len(naf)};")
out.append(f"ZKT_HD constexpr uint32_t miller_naf_nz_word(int i) {{ constexpr uint32_t t[{len(nzw)}] = {{" + ",".join('0x%08xu' % w for w in nzw) + "}; return t[i]; }")
out.append(f"ZKT_HD constexpr uint32_t miller_naf_neg_word(int i) {{ constexpr uint32_t t[{len(ngw)}] = {{" + ",".join('0x%08xu' % w for w in ngw) + "}; return t[i]; }")
out.append(f"static constexpr int MILLER_NBITS = {len(lb)};")
out.append(f"ZKT_HD constexpr uint32_t miller_bits_word(int i) {{ constexpr uint32_t t[{len(words)}] = {{" + ",".join('0x%08xu' % w for w in words) + "}; return t[i]; }")
# the 127-step Miller loop (twisted-ate form, oracle/fast_model.py "short Miller loop"): bits of x^2 (MSB first, leading 1 dropped), the cube root of
# unity BETA with [x^2] P = (BETA x, -y) on G1, and the coefficients of psi = twist o Frobenius o untwist on E'(Fq2)
xb = fm.X2_BITS
xw = [sum(b << j for j, b in enumerate(xb[i:i + 32])) for i in range(0, len(xb), 32)]
out.append("// short Miller loop over x^2 (127 steps, 16 additions): tate = pi^2(eta)^2 conj(eta) for eta = f_{x^2,P}(Q)^((q^12-1)/r), P in G1, Q in G2 (pairing.h)")
out.append(f"static constexpr int MILLER_X2_NBITS = {len(xb)};")
out.append(f"ZKT_HD constexpr uint32_t miller_x2_bits_word(int i) {{ constexpr uint32_t t[{len(xw)}] = {{" + ",".join('0x%08xu' % w for w in xw) + "}; return t[i]; }")
out.append(f"ZKT_HD constexpr uint32_t g1_beta_limb(int i) {{ constexpr uint32_t t[{FQN}] = {arr_w(limbs_w(fm.BETA * (1 << (FQW * FQN)) % Q, FQN, FQW))}; return t[i]; }}   // [x^2] P = (BETA x, -y) on G1")
out.append(f"ZKT_HD constexpr uint32_t g2_psi_x_limb(int c, int i) {{ constexpr uint32_t t[2][{FQN}] = {fq2_arr(fm.PSI_X)}; return t[c][i]; }}   // psi(x, y) = (PSI_X conj(x), PSI_Y conj(y))")
out.append(f"ZKT_HD constexpr uint32_t g2_psi_y_limb(int c, int i) {{ constexpr uint32_t t[2][{FQN}] = {fq2_arr(fm.PSI_Y)}; return t[c][i]; }}")
FR_ROOT = pow(7, (R - 1) >> 32, R)       # 7 generates Fr^*; r - 1 = 2^32 * odd
assert pow(FR_ROOT, 1 << 32, R) == 1 and pow(FR_ROOT, 1 << 31, R) != 1
out.append("// Fr has 2-adicity 32: FR_ROOT = 7^((r-1)/2^32) has order 2^32 (NTT of the Groth16 quotient stage); canonical 32-bit words")
out.append("static constexpr int FR_TWO_ADICITY = 32;")
out.append(f"ZKT_HD constexpr uint32_t fr_root_word(int i) {{ constexpr uint32_t t[8] = {arr_w(limbs_w(FR_ROOT, 8, 32))}; return t[i]; }}")
out.append("}  // namespace zkt")

path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "zk-toolkit_amd", "csrc", "zkt_constants.h")
with open(path, "w") as f:
    f.write("\n".join(out) + "\n")
print("wrote", os.path.normpath(path))
