"""tests/pinocchio_verify_model.py (Verifier::verify on discrete logarithms) against the oracle's line-by-line verifier (zkto_pinocchio_verify, eleven faithful
Tate pairings) on a key and proofs that the oracle's own generator multiplications build from the model's exponents, n_io = 2.  The GPU tests of
zkt_pinocchio_verify_batch (tests/test_gpu_pinocchio_verify_batch.py) then compare with the model at batch sizes the oracle could not serve."""
import ctypes
import numpy as np
import pytest
from zkt_testlib import *
from qap_util import alloc_pinocchio, alloc_pinocchio_proof
import pinocchio_verify_model as M

O = oracle()
N_IO = 2


def _points(exps, g2):
    """generator * e for every e, through the oracle; exponent 0 is the point at infinity"""
    n = len(exps)
    w = G2W if g2 else G1W
    gen = np.zeros((1, w), np.uint64); (O.zkto_g2_generator if g2 else O.zkto_g1_generator)(ptr(gen))
    out = np.zeros((n, w), np.uint64)
    assert (O.zkto_g2_mul_batch if g2 else O.zkto_g1_mul_batch)(ptr(np.repeat(gen, n, axis=0)), ptr(ints_to_arr([e % R for e in exps], 4)), 4, ptr(out), n, 8) == 0
    for i, e in enumerate(exps):
        if e % R == 0: out[i] = 0; out[i, w - 1] = 1
    return out


@pytest.fixture(scope="module")
def setting():
    rng = SplitMix64(4242)
    key = M.random_key(rng, N_IO)
    io = [1, rng.below(R)]
    crs, buf = alloc_pinocchio(4, N_IO, 1, 1)
    for name, field, g2 in (("one2", "one_g2", 1), ("alpha_v", "alpha_v", 1), ("alpha_w", "alpha_w", 0), ("alpha_y", "alpha_y", 1), ("gamma", "gamma", 1),
                            ("beta_gamma", "beta_gamma", 1), ("t", "t", 0)):
        buf[field][:] = _points([key[name]], g2)
    buf["vk_io"][:] = _points(key["vk"], 0); buf["wk_io"][:] = _points(key["wk"], 1); buf["yk_io"][:] = _points(key["yk"], 0)
    return key, io, crs, buf, M.accepting_proof(key, io, rng)


def _oracle(setting, proof):
    key, io, crs, _, _ = setting
    pf, pb = alloc_pinocchio_proof()
    for k, field in M.PROOF_FIELDS.items(): pb[field][:] = _points([proof[k]], field in ("g2_w_mid_s", "h_s"))
    return O.zkto_pinocchio_verify(ctypes.byref(crs), ctypes.byref(pf), ptr(ints_to_arr(io, 4)))


def test_model_accepts_what_the_oracle_accepts(setting):
    key, io, _, _, proof = setting
    assert M.decide(key, proof, io) == 1 and _oracle(setting, proof) == 1


@pytest.mark.parametrize("c", range(5))
def test_model_rejects_at_each_check_like_the_oracle(setting, c):
    key, io, _, _, proof = setting
    bad = M.rejecting_at(proof, c)
    lhs_rhs = M.checks(key, bad, io)
    holds = [(sum(a * b for a, b in l) - sum(a * b for a, b in r)) % R == 0 for l, r in lhs_rhs]
    assert holds == [k != c for k in range(5)]                      # that check alone fails
    assert M.decide(key, bad, io) == 0 and _oracle(setting, bad) == 0


@pytest.mark.parametrize("c", [2, 4])
def test_model_panics_where_the_oracle_panics(setting, c):
    key, io, _, _, proof = setting
    bad = M.panicking_at(proof, c)
    assert M.decide(key, bad, io) == -M.ZKT_ERR_INFINITY == -ZKT_ERR_INFINITY and _oracle(setting, bad) == -2


def test_model_lets_an_earlier_rejection_win_over_a_later_panic(setting):
    key, io, _, _, proof = setting
    bad = M.reject_before_panic(proof)
    assert M.decide(key, bad, io) == 0 and _oracle(setting, bad) == 0
