"""Verifier::verify (pinocchio/verifier.rs:31-85) on discrete logarithms, in python integers.

Every key and proof point is generator * e for a known e, so e(a G1, b G2) = e(G1, G2)^(a b) and the five equalities are equations mod r:
  check 0 (:43-48)  bvwy * gamma = (v + w1 + y) * beta_gamma
  check 1 (:51-55)  av * one2    = v * alpha_v
  check 2 (:56-60)  aw * one2    = alpha_w * w2
  check 3 (:61-65)  ay * one2    = y * alpha_y
  check 4 (:68-84)  (v + sum io vk)(w2 + sum io wk) = t * h + (y + sum io yk) * one2
A pairing argument is the point at infinity exactly when its exponent is 0 mod r; tate() panics on it (rational_function.rs:36,59).  The checks run in this
order and the first one that does not hold returns false, so a panic is the outcome only when every earlier check passed.

key:   dict with one2, alpha_v, alpha_w, alpha_y, gamma, beta_gamma, t (ints) and vk, wk, yk (lists of n_io ints)
proof: dict with v, w1, w2, y, h, av, aw, ay, bvwy (ints)
io:    list of n_io ints, used as the integers they are (an io wire plus r is the same exponent)"""
from zkt_testlib import R

ZKT_ERR_INFINITY = 2
KEY_SCALARS = ("one2", "alpha_v", "alpha_w", "alpha_y", "gamma", "beta_gamma", "t")
PROOF_FIELDS = {"v": "v_mid_s", "w1": "g1_w_mid_s", "w2": "g2_w_mid_s", "y": "y_mid_s", "h": "h_s", "av": "alpha_v_mid_s", "aw": "alpha_w_mid_s", "ay": "alpha_y_mid_s",
                "bvwy": "beta_vwy_mid_s"}
# the proof element that appears in check c and in no other: moving it moves that check alone
OWN = ("bvwy", "av", "aw", "ay", "h")


def sums(key, proof, io):
    dot = lambda pts: sum(a * b for a, b in zip(io, pts))
    return (proof["v"] + dot(key["vk"])) % R, (proof["w2"] + dot(key["wk"])) % R, (proof["y"] + dot(key["yk"])) % R


def checks(key, proof, io):
    """the five equalities as (lhs pairs, rhs pairs), a pair = (G1 exponent, G2 exponent)"""
    v_s, w_s, y_s = sums(key, proof, io)
    vwy = (proof["v"] + proof["w1"] + proof["y"]) % R
    return [([(proof["bvwy"], key["gamma"])], [(vwy, key["beta_gamma"])]),
            ([(proof["av"], key["one2"])], [(proof["v"], key["alpha_v"])]),
            ([(proof["aw"], key["one2"])], [(key["alpha_w"], proof["w2"])]),
            ([(proof["ay"], key["one2"])], [(proof["y"], key["alpha_y"])]),
            ([(v_s, w_s)], [(key["t"], proof["h"]), (y_s, key["one2"])])]


def decide(key, proof, io):
    """1 accept, 0 reject, -ZKT_ERR_INFINITY where the reference panics"""
    for lhs, rhs in checks(key, proof, io):
        if any(a % R == 0 or b % R == 0 for a, b in lhs + rhs): return -ZKT_ERR_INFINITY
        if (sum(a * b for a, b in lhs) - sum(a * b for a, b in rhs)) % R: return 0
    return 1


def random_key(rng, n_io):
    nz = lambda: rng.below(R - 1) + 1
    key = {k: nz() for k in KEY_SCALARS}
    for k in ("vk", "wk", "yk"): key[k] = [nz() for _ in range(n_io)]
    return key


def accepting_proof(key, io, rng):
    """v, w1, w2, y free; the other five solved from their checks.  The draws are repeated until no argument is at infinity."""
    inv = lambda a: pow(a, -1, R)
    while True:
        p = {k: rng.below(R - 1) + 1 for k in ("v", "w1", "w2", "y")}
        v_s, w_s, y_s = sums(key, p, io)
        p["bvwy"] = (p["v"] + p["w1"] + p["y"]) * key["beta_gamma"] % R * inv(key["gamma"]) % R
        p["av"] = p["v"] * key["alpha_v"] % R * inv(key["one2"]) % R
        p["aw"] = key["alpha_w"] * p["w2"] % R * inv(key["one2"]) % R
        p["ay"] = p["y"] * key["alpha_y"] % R * inv(key["one2"]) % R
        p["h"] = (v_s * w_s - y_s * key["one2"]) % R * inv(key["t"]) % R
        if decide(key, p, io) == 1: return p


def rejecting_at(proof, c):
    """the proof with check c, and no other, failing"""
    q = dict(proof); q[OWN[c]] = (q[OWN[c]] + 1) % R or 2
    return q


def panicking_at(proof, c):
    """the proof with an argument of check c, and of no other, at infinity"""
    q = dict(proof); q[OWN[c]] = 0
    return q


def reject_before_panic(proof):
    """check 1 fails and check 2 has an argument at infinity: the reference returns false before it evaluates the panic"""
    return panicking_at(rejecting_at(proof, 1), 2)
