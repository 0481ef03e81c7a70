"""CPU checks of tests/stream_order_model.py: every `void* stream` function of include/zkt.h is tied to a delayed-producer case of
tests/test_gpu_stream_order.py (or carries the reason it needs none), every case named there exists, and the constants of
zk-toolkit_amd/csrc/zkt_msm_handle.cpp the pipeline cases are built on still read as the model restates them."""
import os, re
import pytest
import stream_order_model as S


def test_the_header_parser_finds_the_stream_functions():
    fns = S.stream_functions()
    assert len(fns) == len(set(fns)) == 28, fns
    assert "zkt_tate_batch_dev" in fns and "zkt_secp_jac_sum_dev" in fns and "zkt_g2_msm_sharded" in fns
    assert "zkt_g1_msm_collect" not in fns and "zkt_groth16_prove_r1cs_dev" not in fns      # no stream parameter


def test_every_stream_function_has_a_case_or_an_exempt_reason():
    assert S.table_problems() == []
    assert len(S.case_ids()) == 25 and sum(1 for k, _ in S.TABLE.values() if k == "exempt") == 3


def test_a_new_stream_prototype_is_noticed(tmp_path):
    with open(S.HEADER) as f:
        text = f.read()
    marker = "int zkt_fq_mul_batch_dev("
    assert text.count(marker) == 1
    for proto in ("int zkt_fr_mul_batch_dev(const uint64_t* dev_a, const uint64_t* dev_b, uint64_t* dev_out, size_t n, void* stream);\n",
                  "int zkt_secp_mul_batch_dev(const zkt_secp_affine* dev_points, const uint64_t* dev_scalars, int scalar_limbs,\n"
                  "                           zkt_secp_affine* dev_out, size_t n, void *stream);\n"):
        h = tmp_path / "zkt.h"
        h.write_text(text.replace(marker, proto + marker))
        name = re.search(r"zkt_[a-z0-9_]+", proto).group(0)
        assert name in S.stream_functions(str(h))
        assert any(p.startswith(name + ":") for p in S.table_problems(str(h)))


def test_a_missing_or_stray_case_is_noticed(tmp_path):
    with open(S.GPU_MODULE) as f:
        text = f.read()
    assert text.count('@case("secp_jac_sum_dev")') == 1
    m = tmp_path / "gpu_module.py"
    m.write_text(text.replace('@case("secp_jac_sum_dev")', '@case("secp_jac_sum")'))
    bad = S.table_problems(module=str(m))
    assert any(p.startswith("zkt_secp_jac_sum_dev:") for p in bad) and any("'secp_jac_sum'" in p for p in bad)


def test_the_gpu_module_runs_the_cases_of_the_table():
    """the parametrised test of the GPU module takes its ids from the table, so a case cannot be defined and left out of the run"""
    with open(S.GPU_MODULE) as f:
        text = f.read()
    assert '@pytest.mark.parametrize("cid", S.case_ids())' in text


def test_the_constants_match_the_source():
    for what, want, found in S.source_line_counts():
        assert found == want, f"{what}: the line the model restates occurs {found} times in the source, expected {want}"
    assert S.MSM_SLOTS == S.NTAIL, "the small-path case gives every slot a reduce stream of its own"


def test_slot_streams_of_the_model():
    n_small, n_large = (1 << S.LARGE_LOG2) - 1, 1 << S.LARGE_LOG2
    assert not S.large(n_small) and S.large(n_large)
    assert sorted({S.tail_stream_index(n_small, k) for k in range(S.MSM_SLOTS)}) == list(range(S.NTAIL))
    assert [S.tail_stream_index(n_large, k) for k in range(S.MSM_SLOTS)] == [0, 1] * (S.MSM_SLOTS // 2)


def test_the_groth16_device_wire_forms_say_which_stream_they_expect():
    """they take device wires and no stream: the header has to say where the wires must be ready"""
    with open(S.HEADER) as f:
        text = f.read()
    assert "zkt_groth16_prove_r1cs_dev, _submit and _partials take no stream" in text
    with open(os.path.join(S.ROOT, "zk-toolkit_amd", "csrc", "zkt_groth16_r1cs.hip")) as f:
        src = f.read()
    # what the sentence rests on: the wires are copied on the key's own non-blocking stream, behind nothing of the caller's
    assert "HIPCHK(hipStreamCreateWithFlags(&pk->s, hipStreamNonBlocking));" in src
    assert "HIPCHK(hipMemcpyAsync(pk->wires_c.p, wires, rows * FRB, wires_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));" in src
