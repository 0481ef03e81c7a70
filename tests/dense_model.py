"""The two dense trusted-setup protocols on the EXPONENTS, in python integers: every CRS element and every proof point of zkt_groth16_setup / zkt_groth16_prove
(groth16/zktoolkit_based/crs.rs:59-135, prover.rs:96-147) and of zkt_pinocchio_setup / zkt_pinocchio_prove / zkt_pinocchio_prove_resident (pinocchio/crs.rs:86-140,
prover.rs:124-161) is generator * scalar, and with the trapdoor known the scalar is a few lines of arithmetic mod r.  Independent of the HIP path and of the oracle's
restatement; tests/test_dense_model.py ties it to that restatement at the reference's toy circuits, tests/test_gpu_dense_protocols.py compares the library with it.

Inputs are flat row-major lists of 256-bit integers (rows x n coefficients, low degree first) exactly as the C ABI takes them; every value is reduced mod r first.
Outputs map a field name of zkt_groth16_crs / zkt_pinocchio_crs / zkt_pinocchio_proof to its list of scalars mod r; *_GROUPS gives the group of each field.

The module also holds the case lists of tests/test_gpu_dense_protocols.py and a census: `CELLS` names every block edge, empty slice and verifier route those cases are
meant to reach, `census(case)` says which ones a case reaches with the block widths and PIN_FAST_IO that the library SOURCE holds (library_constants()), so a changed
constant breaks tests/test_dense_model.py instead of silently moving an edge away from the cases."""
import os, re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zk-toolkit_amd", "csrc")
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001

# ---- the constants the case lists were chosen for (test_dense_model compares them with the source) --------------------------------------
LINCOMB_TPB = 256           # k_lincomb<FrC>: lanes over n (zkt_groth16.hip)
POWSEQ_TPB = 256            # k_pin_powseq: lanes over max_degree (zkt_pinocchio.hip)
EVAL_ROWS_TPB = 64          # k_eval_rows: lanes over rows (zkt_fr_vec.hip)
PIN_SCALARS_TPB = 64        # k_pin_scalars: lanes over rows (zkt_pinocchio.hip)
GENMUL_TPB = 64             # k_generator_mul: lanes over elements (zkt_group.hip)
PIN_FAST_IO = 12            # zkt_pinocchio_verify: up to this many io wires through the per-key tables
PIN_TABLE_SLOTS = 2         # keys whose tables are kept


def model_constants():
    return {"LINCOMB_TPB": LINCOMB_TPB, "POWSEQ_TPB": POWSEQ_TPB, "EVAL_ROWS_TPB": EVAL_ROWS_TPB, "PIN_SCALARS_TPB": PIN_SCALARS_TPB, "GENMUL_TPB": GENMUL_TPB,
            "PIN_FAST_IO": PIN_FAST_IO, "PIN_TABLE_SLOTS": PIN_TABLE_SLOTS}


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _kernel_width(text, kernel, default_tpb):
    """lanes per block of a one-lane-per-item kernel: its launch bounds, its index line and every launch of it must agree"""
    m = re.findall(r"__launch_bounds__\((\d+)\) %s\([^{]*\{\s*(?:const )?size_t \w+ = \(size_t\)blockIdx\.x \* (\d+) \+ threadIdx\.x;" % kernel, text)
    assert len(m) == 1 and m[0][0] == m[0][1], \
        f"{kernel}: expected one definition `__launch_bounds__(W) {kernel}(...) {{ size_t i = (size_t)blockIdx.x * W + threadIdx.x;` with one W, found {m}; " \
        "if the kernel was only reformatted, update this pattern, if its width changed, choose new shapes for the case lists below"
    w = int(m[0][0])
    launches = re.findall(r"hipLaunchKernelGGL\(%s(?:<\w+>)?, dim3\(grid_blocks\(\w+(?:, (\d+))?\)\), dim3\((\d+)\)" % kernel, text)
    assert launches, f"{kernel}: no launch of the form `hipLaunchKernelGGL({kernel}, dim3(grid_blocks(count[, W])), dim3(W)` found; if the launch was only reformatted, update this pattern"
    for grid, block in launches:
        assert int(block) == w and int(grid or default_tpb) == w, f"{kernel}: a launch's grid or block width differs from the kernel's {w}: {launches}"
    return w


def library_constants():
    """the same constants as the library source writes them"""
    d = re.findall(r"grid_blocks\(size_t n, unsigned tpb = (\d+)\)", _read("zkt_internal.h"))
    assert len(d) == 1, f"zkt_internal.h: expected one `grid_blocks(size_t n, unsigned tpb = N)`, found {d}"
    d = int(d[0])
    proto, pin = _read("zkt_groth16.hip"), _read("zkt_pinocchio.hip")
    fast = re.findall(r"constexpr size_t PIN_FAST_IO = (\d+);", pin)
    slots = re.findall(r"PinTables tab\[(\d+)\];", pin)
    assert len(fast) == 1 and len(slots) == 1, f"zkt_pinocchio.hip: expected one `constexpr size_t PIN_FAST_IO = N;` and one `PinTables tab[N];`, found {fast} and {slots}"
    assert len(re.findall(r"if \(c->n_io <= PIN_FAST_IO\)", pin)) == 1, "zkt_pinocchio_verify no longer chooses its path by `if (c->n_io <= PIN_FAST_IO)`: restate the rule here and in census()"
    assert len(re.findall(r"FixedTables \{ const uint32_t\* point\[%s\]; uint32_t\* table\[%s\]; int n; \};" % (fast[0], fast[0]), _read("zkt_internal.h"))) == 1, \
        "zkt_internal.h: FixedTables no longer holds exactly PIN_FAST_IO points per launch"
    return {"LINCOMB_TPB": _kernel_width(proto, "k_lincomb", d), "POWSEQ_TPB": _kernel_width(pin, "k_pin_powseq", d),
            "EVAL_ROWS_TPB": _kernel_width(_read("zkt_fr_vec.hip"), "k_eval_rows", d), "PIN_SCALARS_TPB": _kernel_width(pin, "k_pin_scalars", d),
            "GENMUL_TPB": _kernel_width(_read("zkt_group.hip"), "k_generator_mul", d), "PIN_FAST_IO": int(fast[0]), "PIN_TABLE_SLOTS": int(slots[0])}


# ---- arithmetic ------------------------------------------------------------------------------------------------------------------------
def _red(xs):
    return [int(x) % R for x in xs]


def horner(p, x):
    """Polynomial::eval_at (field/polynomial.rs:240-249)"""
    acc = 0
    for c in reversed(p): acc = (acc * x + c) % R
    return acc


def t_at(x, n):
    """t(x) = prod_{i=1..n} (x - i): QAP::build_t(f, n).eval_at(x) (qap/qap.rs:115-135), what fr_t_at computes (csrc/fr_vec.h)"""
    t = 1
    for i in range(1, n + 1): t = t * (x - i) % R
    return t


def _row_evals(P, rows, n, x):
    assert len(P) == rows * n, (len(P), rows, n)
    P = _red(P)
    return [horner(P[i * n:(i + 1) * n], x) for i in range(rows)]


def _combine(P, a, rows, n):
    """sum_i a_i P_i, coefficient by coefficient (prover.rs:107-117 done in Fr first)"""
    P = _red(P)
    return [sum(a[i] * P[i * n + k] for i in range(rows)) % R for k in range(n)]


def _dot(a, b):
    assert len(a) == len(b), (len(a), len(b))
    return sum(x * y for x, y in zip(a, b)) % R


G16_GROUPS = {"g1_alpha": "g1", "g1_beta": "g1", "g1_delta": "g1", "g1_xi": "g1", "g1_uvw_stmt": "g1", "g1_uvw_wit": "g1", "g1_xt_by_delta": "g1",
              "g2_beta": "g2", "g2_gamma": "g2", "g2_delta": "g2", "g2_xi": "g2"}          # the twelfth field, gt_alpha_beta, is tate(g1_alpha, g2_beta) (crs.rs:137-139)


def groth16_crs(ui, vi, wi, n, l, m, alpha, beta, gamma, delta, x):
    """CRS::new (crs.rs:59-135) on the exponents"""
    alpha, beta, gamma, delta, x = _red([alpha, beta, gamma, delta, x])
    assert n >= 1 and l <= m and all((alpha, beta, gamma, delta, x)), "rand_elem(true) draws no zero"
    rows = m + 1
    ue, ve, we = (_row_evals(P, rows, n, x) for P in (ui, vi, wi))
    ginv, dinv = pow(gamma, -1, R), pow(delta, -1, R)
    y = [(beta * ue[i] + alpha * ve[i] + we[i]) * (ginv if i <= l else dinv) % R for i in range(rows)]      # calc_uvw_div! crs.rs:65-83
    xi = [pow(x, k, R) for k in range(n)]                                                                  # calc_n_pows! crs.rs:88-104
    td = t_at(x, n) * dinv % R
    return {"g1_alpha": [alpha], "g1_beta": [beta], "g1_delta": [delta], "g1_xi": xi, "g1_uvw_stmt": y[:l + 1], "g1_uvw_wit": y[l + 1:],
            "g1_xt_by_delta": [xk * td % R for xk in xi], "g2_beta": [beta], "g2_gamma": [gamma], "g2_delta": [delta], "g2_xi": list(xi)}


def groth16_proof(crs, ui, vi, wires, h, r, s, n, l, m):
    """Prover::prove (prover.rs:96-147) on the exponents of the model's own CRS: {"A", "B", "C"}"""
    rows = m + 1
    a, h = _red(wires), _red(h)
    r, s = _red([r, s])
    assert len(a) == rows and len(h) <= n
    U, V = _combine(ui, a, rows, n), _combine(vi, a, rows, n)
    delta = crs["g1_delta"][0]
    A = (crs["g1_alpha"][0] + _dot(U, crs["g1_xi"]) + r * delta) % R                     # :118
    B = (crs["g2_beta"][0] + _dot(V, crs["g2_xi"]) + s * crs["g2_delta"][0]) % R         # :119
    B1 = (crs["g1_beta"][0] + _dot(V, crs["g1_xi"]) + s * delta) % R                     # :120
    C = (_dot(a[l + 1:], crs["g1_uvw_wit"]) + _dot(h, crs["g1_xt_by_delta"][:len(h)]) + s * A + r * B1 - r * s * delta) % R      # :127-140
    return {"A": A, "B": B, "C": C}


PROOF16_GROUPS = {"A": "g1", "B": "g2", "C": "g1"}

PIN_MID = ["vk_mid", "g1_wk_mid", "g2_wk_mid", "yk_mid", "alpha_vk_mid", "alpha_wk_mid", "alpha_yk_mid", "beta_vwy_k_mid"]      # the seven columns and g2_wk
PIN_IO = ["vk_io", "wk_io", "yk_io"]
PIN_SINGLES = ["one_g1", "one_g2", "alpha_v", "alpha_w", "alpha_y", "gamma", "beta_gamma", "t", "alpha_v_t", "alpha_y_t", "beta_t"]
PIN_GROUPS = {k: "g1" for k in PIN_MID + PIN_IO + PIN_SINGLES}
PIN_GROUPS.update({k: "g2" for k in ("g2_wk_mid", "si", "wk_io", "one_g2", "alpha_v", "alpha_y", "gamma", "beta_gamma")})
PIN_PROOF_GROUPS = {"v_mid_s": "g1", "g1_w_mid_s": "g1", "g2_w_mid_s": "g2", "y_mid_s": "g1", "h_s": "g2", "alpha_v_mid_s": "g1", "alpha_w_mid_s": "g1",
                    "alpha_y_mid_s": "g1", "beta_vwy_mid_s": "g1"}


def pinocchio_crs(vi, wi, yi, n, n_io, n_mid, max_degree, rnd):
    """CRS::new (pinocchio/crs.rs:58-140) on the exponents; rnd = r_v, r_w, alpha_v, alpha_w, alpha_y, beta, gamma, s"""
    r_v, r_w, a_v, a_w, a_y, beta, gamma, s = _red(rnd)
    assert n >= 1 and max_degree >= 1 and n_io + n_mid >= 1 and all((r_v, r_w, a_v, a_w, a_y, beta, gamma, s)), "rand_elem(true) draws no zero"
    rows = n_io + n_mid
    r_y = r_v * r_w % R                                                                  # crs.rs:67
    v = [r_v * e % R for e in _row_evals(vi, rows, n, s)]
    w = [r_w * e % R for e in _row_evals(wi, rows, n, s)]
    y = [r_y * e % R for e in _row_evals(yi, rows, n, s)]
    T = r_y * t_at(s, n) % R                                                             # :120
    return {"vk_mid": v[n_io:], "g1_wk_mid": w[n_io:], "g2_wk_mid": w[n_io:], "yk_mid": y[n_io:],                                        # :86-108
            "alpha_vk_mid": [a_v * e % R for e in v[n_io:]], "alpha_wk_mid": [a_w * e % R for e in w[n_io:]], "alpha_yk_mid": [a_y * e % R for e in y[n_io:]],
            "beta_vwy_k_mid": [beta * (v[i] + w[i] + y[i]) % R for i in range(n_io, rows)],
            "si": [pow(s, k, R) for k in range(max_degree)],                                                                           # :98-99
            "one_g1": [1], "one_g2": [1], "alpha_v": [a_v], "alpha_w": [a_w], "alpha_y": [a_y], "gamma": [gamma], "beta_gamma": [gamma * beta % R],   # :110-118
            "t": [T], "vk_io": v[:n_io], "wk_io": w[:n_io], "yk_io": y[:n_io],                                                           # :120-124
            "alpha_v_t": [T * a_v % R], "alpha_y_t": [T * a_y % R], "beta_t": [T * beta % R]}                                            # :138-140


def pinocchio_proof(crs, wires, h, delta_v, delta_y, n_io):
    """Prover::prove (pinocchio/prover.rs:124-161) on the exponents of the model's own CRS: the nine proof points"""
    a, h = _red(wires), _red(h)
    dv, dy = _red([delta_v, delta_y])
    assert len(h) <= len(crs["si"]) and len(a) == n_io + len(crs["vk_mid"])
    mid = a[n_io:]
    t, bt = crs["t"][0], crs["beta_t"][0]
    w_s = (_dot(mid, crs["g2_wk_mid"]) + _dot(a[:n_io], crs["wk_io"])) % R                                     # :155-159
    return {"v_mid_s": (t * dv + _dot(mid, crs["vk_mid"])) % R, "g1_w_mid_s": _dot(mid, crs["g1_wk_mid"]), "g2_w_mid_s": _dot(mid, crs["g2_wk_mid"]),
            "y_mid_s": (t * dy + _dot(mid, crs["yk_mid"])) % R,
            "alpha_v_mid_s": (crs["alpha_v_t"][0] * dv + _dot(mid, crs["alpha_vk_mid"])) % R, "alpha_w_mid_s": _dot(mid, crs["alpha_wk_mid"]),
            "alpha_y_mid_s": (crs["alpha_y_t"][0] * dy + _dot(mid, crs["alpha_yk_mid"])) % R,
            "beta_vwy_mid_s": (bt * dv + bt * dy + _dot(mid, crs["beta_vwy_k_mid"])) % R,                      # :131
            "h_s": (_dot(h, crs["si"][:len(h)]) + w_s * dv - crs["one_g2"][0] * dy) % R}                       # :153-160


# ---- seeded inputs -----------------------------------------------------------------------------------------------------------------------
class _Rng:
    """SplitMix64, so that the inputs do not depend on a library's generator"""

    def __init__(self, seed): self.s = seed & 0xFFFFFFFFFFFFFFFF

    def u64(self):
        self.s = (self.s + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
        return z ^ (z >> 31)

    def fr(self):
        """uniform in [0, r) (a 320-bit draw reduced)"""
        return sum(self.u64() << (64 * i) for i in range(5)) % R

    def nonzero(self): return self.fr() % (R - 1) + 1


TOP = (1 << 256) - 1
NONCANONICAL = [R, R + 1, 2 * R, 2 * R + 5, TOP, TOP - 1]          # values >= r that fit four limbs; the first and third reduce to zero


def _lift(rng, v):
    """a four-limb integer >= r that is v mod r: v + r always fits (2r < 2^256), v + 2r for the smaller v"""
    return v + (2 * R if v + 2 * R <= TOP and rng.u64() % 2 else R)


def _noncanonical_vector(rng, count, edges=0):
    """`count` four-limb integers >= r: lifted random values, one in four a fixed edge value, and the last `edges` entries the edge values in turn (2^256 - 1 last)"""
    out = [NONCANONICAL[rng.u64() % len(NONCANONICAL)] if rng.u64() % 4 == 0 else _lift(rng, rng.fr()) for _ in range(count)]
    for j in range(min(edges, count)): out[count - 1 - j] = NONCANONICAL[(4 + j) % len(NONCANONICAL)]
    return out


def _noncanonical_matrix(rng, rows, n):
    """rows x n coefficients >= r; row 0 and the last row are made entirely of the fixed edge values"""
    out = []
    for i in range(rows):
        if i in (0, rows - 1): out += [NONCANONICAL[(i + k) % len(NONCANONICAL)] for k in range(n)]
        else: out += _noncanonical_vector(rng, n)
    return out


def _noncanonical_nonzero(rng, k):
    """a trapdoor >= r that is not zero mod r: r + 1, 2^256 - 1, then lifted random ones"""
    return [R + 1, TOP][k] if k < 2 else _lift(rng, rng.nonzero())


def groth16_inputs(rows, n, l, seed, noncanonical=False):
    """seeded dense ui, vi, wi (rows x n), trapdoors [alpha, beta, gamma, delta, x], wires, h (n coefficients), r, s.  Setup and prove are linear algebra on
    the exponents, so no satisfiable circuit is needed."""
    rng = _Rng(seed)
    if noncanonical:
        mats = [_noncanonical_matrix(rng, rows, n) for _ in range(3)]
        trap = [_noncanonical_nonzero(rng, k) for k in range(5)]
        wires, h = _noncanonical_vector(rng, rows, 6), _noncanonical_vector(rng, n, 2)
        r, s = R + 1 + rng.fr() % 1000, TOP - rng.fr() % 1000
    else:
        mats = [[rng.fr() for _ in range(rows * n)] for _ in range(3)]
        trap = [rng.nonzero() for _ in range(5)]
        wires, h = [rng.fr() for _ in range(rows)], [rng.fr() for _ in range(n)]
        r, s = rng.nonzero(), rng.nonzero()
    return {"ui": mats[0], "vi": mats[1], "wi": mats[2], "trap": trap, "wires": wires, "h": h, "r": r, "s": s}


def pinocchio_inputs(n_io, n_mid, n, max_degree, seed, noncanonical=False):
    """seeded dense vi, wi, yi ((n_io + n_mid) x n), rnd (8 values), wires, h (max_degree coefficients), delta_v, delta_y"""
    rng = _Rng(seed); rows = n_io + n_mid
    if noncanonical:
        mats = [_noncanonical_matrix(rng, rows, n) for _ in range(3)]
        rnd = [_noncanonical_nonzero(rng, k) for k in range(8)]
        wires, h = _noncanonical_vector(rng, rows, 6), _noncanonical_vector(rng, max_degree, 6)
        dv, dy = TOP - rng.fr() % 1000, R + 1 + rng.fr() % 1000
    else:
        mats = [[rng.fr() for _ in range(rows * n)] for _ in range(3)]
        rnd = [rng.nonzero() for _ in range(8)]
        wires, h = [rng.fr() for _ in range(rows)], [rng.fr() for _ in range(max_degree)]
        dv, dy = rng.nonzero(), rng.nonzero()
    return {"vi": mats[0], "wi": mats[1], "yi": mats[2], "rnd": rnd, "wires": wires, "h": h, "delta_v": dv, "delta_y": dy}


# ---- the GPU cases ------------------------------------------------------------------------------------------------------------------------
# Groth16: (m + 1, n, l).  The smallest shapes that cross each block edge once.
G16_SHAPES = [(1, 1, 0), (63, 255, 0), (64, 256, 63), (65, 257, 3), (129, 2, 64)]
G16_ZERO_WIRES_SHAPE = (63, 255, 0)
G16_NONCANONICAL_SHAPE = (129, 2, 64)
# Pinocchio: (n_io, n_mid, n, max_degree)
PIN_SHAPES = [(0, 1, 1, 1), (2, 0, 2, 3), (1, 62, 2, 255), (12, 52, 5, 256), (13, 52, 4, 257), (0, 129, 2, 2)]
PIN_NONCANONICAL_SHAPE = (1, 62, 2, 255)
VERIFY_IO = [0, 1, 12, 13, 20]
VERIFY_SEQUENCE = [(12, 0), (2, 1), (0, 2), (12, 3), (13, 4), (2, 1), (12, 0)]      # (n_io, key): keys 0 and 3 differ in their randomness only
ZERO_MOD_R = [0, R, 2 * R]


def _h_lens(top):
    return sorted({0, 1, top}) if top >= 1 else [0]


def g16_cases():
    out = [{"kind": "g16", "shape": sh, "h_lens": _h_lens(sh[1]), "zero_wires": sh == G16_ZERO_WIRES_SHAPE, "noncanonical": False} for sh in G16_SHAPES]
    out.append({"kind": "g16", "shape": G16_NONCANONICAL_SHAPE, "h_lens": [G16_NONCANONICAL_SHAPE[1]], "zero_wires": False, "noncanonical": True})
    return out


def pin_cases():
    """one-shot prover: h_len 0 and max_degree; resident prover: the same and one length strictly between when there is one"""
    out = []
    for sh, nonc in [(sh, False) for sh in PIN_SHAPES] + [(PIN_NONCANONICAL_SHAPE, True)]:
        deg = sh[3]
        out.append({"kind": "pin", "shape": sh, "h_lens": sorted({0, deg}), "resident_h_lens": sorted({0, deg} | ({deg // 2} if deg >= 2 else set())), "noncanonical": nonc})
    return out


def verify_cases():
    return [{"kind": "verify", "n_io": k} for k in VERIFY_IO] + [{"kind": "verify_sequence", "sequence": list(VERIFY_SEQUENCE)}]


def trapdoor_cases():
    return [{"kind": "g16_zero_trapdoor", "values": list(ZERO_MOD_R), "positions": 5}, {"kind": "pin_zero_rnd", "values": list(ZERO_MOD_R), "positions": 8}]


def all_cases():
    return g16_cases() + pin_cases() + verify_cases() + trapdoor_cases()


def case_id(c):
    if c["kind"] in ("g16", "pin"): return "x".join(str(v) for v in c["shape"]) + ("-noncanonical" if c["noncanonical"] else "")
    if c["kind"] == "verify": return "io%d" % c["n_io"]
    return c["kind"]


CELLS = [
    # k_lincomb<FrC> over n
    "lincomb_first_block_only", "lincomb_block_full", "lincomb_second_block",
    # k_eval_rows / k_generator_mul over the rows of either setup, k_pin_scalars over Pinocchio's
    "g16_rows_one", "g16_rows_below_block", "g16_rows_block_full", "g16_rows_second_block_one_lane", "g16_rows_third_block",
    "pin_rows_one", "pin_rows_below_block", "pin_rows_block_full", "pin_rows_second_block_one_lane", "pin_rows_third_block",
    # k_generator_mul over the n powers (xi, xt_by_delta, g2_xi) and the max_degree powers (si)
    "g16_powers_one", "g16_powers_many_blocks_ragged", "g16_powers_blocks_full", "pin_powers_one", "pin_powers_many_blocks_ragged", "pin_powers_blocks_full",
    # k_pin_powseq over max_degree
    "powseq_first_block_only", "powseq_block_full", "powseq_second_block",
    # the slices of the CRS buffers
    "g16_l_zero", "g16_l_equals_m", "g16_one_wire", "g16_divisor_switch_at_block_edge", "pin_no_io", "pin_no_mid", "pin_io_at_block_edge",
    # the provers
    "g16_h_empty", "g16_h_one", "g16_h_full", "g16_h_too_long", "g16_wires_zero", "g16_noncanonical",
    "pin_h_empty", "pin_h_full", "pin_h_padded", "pin_resident_twice", "pin_h_too_long", "pin_noncanonical",
    # zkt_pinocchio_verify
    "verify_tables_no_io", "verify_tables_one_io", "verify_tables_full", "verify_table_free_first", "verify_table_free_beyond", "verify_sums_most_terms",
    "verify_cache_two_sizes", "verify_cache_hit", "verify_cache_evict", "verify_cache_rebuild", "verify_table_free_between_tables", "verify_no_io_between_tables",
    # trapdoors that are zero mod r
    "g16_trapdoor_zero_mod_r", "pin_rnd_zero_mod_r",
]


def _count_cells(prefix, count, tpb):
    """the cells a one-lane-per-item launch over `count` items reaches"""
    c = set()
    if count == 1: c.add(prefix + "_one")
    if 1 < count < tpb: c.add(prefix + "_below_block")
    if count == tpb: c.add(prefix + "_block_full")
    if count == tpb + 1: c.add(prefix + "_second_block_one_lane")
    if count > 2 * tpb: c.add(prefix + "_third_block")
    return c


def _power_cells(prefix, count, tpb):
    c = set()
    if count == 1: c.add(prefix + "_one")
    if count > 2 * tpb and count % tpb: c.add(prefix + "_many_blocks_ragged")
    if count >= 2 * tpb and count % tpb == 0: c.add(prefix + "_blocks_full")
    return c


def _wide_cells(prefix, count, tpb):
    c = set()
    if count < tpb: c.add(prefix + "_first_block_only")
    if count == tpb: c.add(prefix + "_block_full")
    if count > tpb: c.add(prefix + "_second_block")
    return c


def cache_walk(sequence, fast_io, slots):
    """the table cache of zkt_pinocchio_verify over a sequence of (n_io, key), started EMPTY: least recently used of `slots` entries, no entry for n_io == 0 or
    n_io > fast_io.  Returns one of "none", "free", "build", "hit", "evict", "rebuild" per step.  In the GPU module the cache is not empty when the sequence starts
    (it holds the keys of the tests before it), so there the first `slots` "build" steps are evictions of those keys; every later step is as the walk says, and the
    hit, evict and rebuild steps the census counts all come after them."""
    held, seen, out, clock = {}, set(), [], 0
    for n_io, key in sequence:
        clock += 1
        if n_io == 0: out.append("none"); continue
        if n_io > fast_io: out.append("free"); continue
        if key in held: held[key] = clock; out.append("hit"); continue
        what = "build"
        if len(held) == slots:
            del held[min(held, key=held.get)]; what = "evict"
        if key in seen: what = "rebuild"
        held[key] = clock; seen.add(key); out.append(what)
    return out


def census(case, k=None):
    """the cells of CELLS that one GPU case reaches, with the constants `k` (default: the library source's)"""
    k = library_constants() if k is None else k
    c = set()
    if case["kind"] == "g16":
        rows, n, l = case["shape"]; m = rows - 1
        c |= _wide_cells("lincomb", n, k["LINCOMB_TPB"])
        assert k["EVAL_ROWS_TPB"] == k["GENMUL_TPB"], "the row cells assume one width for k_eval_rows and k_generator_mul"
        c |= _count_cells("g16_rows", rows, k["EVAL_ROWS_TPB"]) | _power_cells("g16_powers", n, k["GENMUL_TPB"])
        if l == 0: c.add("g16_l_zero")
        if l == m: c.add("g16_l_equals_m")
        if m == 0: c.add("g16_one_wire")
        if l < m and l and l % k["EVAL_ROWS_TPB"] == 0: c.add("g16_divisor_switch_at_block_edge")      # the last statement row is lane 0 of a block
        if 0 in case["h_lens"]: c.add("g16_h_empty")
        if 1 in case["h_lens"]: c.add("g16_h_one")
        if n in case["h_lens"]: c.add("g16_h_full")
        c.add("g16_h_too_long")
        if case["zero_wires"]: c.add("g16_wires_zero")
        if case["noncanonical"]: c.add("g16_noncanonical")
    elif case["kind"] == "pin":
        n_io, n_mid, n, deg = case["shape"]; rows = n_io + n_mid
        assert k["EVAL_ROWS_TPB"] == k["GENMUL_TPB"] == k["PIN_SCALARS_TPB"], "the row cells assume one width for k_eval_rows, k_pin_scalars and k_generator_mul"
        c |= _count_cells("pin_rows", rows, k["PIN_SCALARS_TPB"]) | _power_cells("pin_powers", deg, k["GENMUL_TPB"]) | _wide_cells("powseq", deg, k["POWSEQ_TPB"])
        if n_io == 0: c.add("pin_no_io")
        if n_mid == 0: c.add("pin_no_mid")
        if n_io and n_mid and rows in (k["PIN_SCALARS_TPB"], k["PIN_SCALARS_TPB"] + 1): c.add("pin_io_at_block_edge")
        if 0 in case["h_lens"] and 0 in case["resident_h_lens"]: c.add("pin_h_empty")
        if deg in case["h_lens"] and deg in case["resident_h_lens"]: c.add("pin_h_full")
        if any(0 < x < deg for x in case["resident_h_lens"]): c.add("pin_h_padded")
        c |= {"pin_resident_twice", "pin_h_too_long"}
        if case["noncanonical"]: c.add("pin_noncanonical")
    elif case["kind"] == "verify":
        n_io, fast = case["n_io"], k["PIN_FAST_IO"]
        if n_io == 0: c.add("verify_tables_no_io")
        if n_io == 1: c.add("verify_tables_one_io")
        if n_io == fast: c |= {"verify_tables_full", "verify_sums_most_terms"}
        if n_io == fast + 1: c.add("verify_table_free_first")
        if n_io > fast + 1: c.add("verify_table_free_beyond")
    elif case["kind"] == "verify_sequence":
        seq = case["sequence"]; walk = cache_walk(seq, k["PIN_FAST_IO"], k["PIN_TABLE_SLOTS"])
        tabled = [n_io for (n_io, _), w in zip(seq, walk) if w not in ("none", "free")]
        if len(set(tabled)) >= 2: c.add("verify_cache_two_sizes")
        for w in ("hit", "evict", "rebuild"):
            if w in walk: c.add("verify_cache_" + w)
        for name, w in (("verify_table_free_between_tables", "free"), ("verify_no_io_between_tables", "none")):
            if any(x == w and set(walk[:i]) & {"build", "evict", "rebuild"} and set(walk[i + 1:]) & {"hit", "evict", "rebuild"} for i, x in enumerate(walk)): c.add(name)
    elif case["kind"] == "g16_zero_trapdoor":
        if case["values"] == ZERO_MOD_R and case["positions"] == 5: c.add("g16_trapdoor_zero_mod_r")
    elif case["kind"] == "pin_zero_rnd":
        if case["values"] == ZERO_MOD_R and case["positions"] == 8: c.add("pin_rnd_zero_mod_r")
    else:
        raise ValueError(case["kind"])
    return c


def gpu_case_census(k=None):
    k = library_constants() if k is None else k
    c = set()
    for case in all_cases(): c |= census(case, k)
    return c


# ---- expected bytes: generator * scalar through the oracle's threaded batch multiplications ---------------------------------------------------
ORACLE_THREADS = 16
_points = {}        # (group, scalar) -> the point's bytes: cases share most of their singles, and a case's two provers share everything


def expected_points(O, group, scalars):
    """(len(scalars), 13 | 25) u64: generator * scalar in the include/zkt.h layout"""
    import numpy as np
    from zkt_testlib import ptr, ints_to_arr, G1W, G2W
    W = G1W if group == "g1" else G2W
    todo = sorted({s for s in scalars if (group, s) not in _points})
    if todo:
        g = np.zeros((1, W), np.uint64); getattr(O, "zkto_%s_generator" % group)(ptr(g))
        out = np.zeros((len(todo), W), np.uint64)
        assert getattr(O, "zkto_%s_mul_batch" % group)(ptr(np.repeat(g, len(todo), axis=0)), ptr(ints_to_arr(todo, 4)), 4, ptr(out), len(todo), ORACLE_THREADS) == 0
        for s, row in zip(todo, out): _points[(group, s)] = row.copy()
    return np.array([_points[(group, s)] for s in scalars], np.uint64).reshape(len(scalars), W)
