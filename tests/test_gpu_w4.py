"""`-m gpu`: W4A16 (MXFP4 decoder weights) on the device — the cases of tests/w4_cases.py through libvcoder_hip.so (and the fp16-operand
library where the format's bytes must agree), the decoder linears of the 7b / 13b models at their true shapes, and the engine with
weight format 'w4a16'."""
import pytest

import kernel_cases as kc
import w4_cases as w4

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    return kc.HipBackend()


@pytest.fixture(scope="module")
def be16():
    return kc.HipBackend("fp16")


@pytest.mark.parametrize("N,K", [(16, 128), (48, 384)])
def test_quantizer_matches_host(be, be16, N, K):
    """the byte comparison that confirms the nibble order: device nibbles, scale bytes and rewrite against numpy, both libraries"""
    w4.check_quantizer(be, N, K, seed=N)
    w4.check_quantizer(be16, N, K, seed=N + 1)


@pytest.mark.parametrize("epi", [0, 1, 2, 3])
def test_gemv_w4(be, epi):
    for i, (M, N, K, nt) in enumerate(w4.GEMV_CASES):
        w4.check_gemv(be, M, N, K, epi, norm=bool((i + epi) & 1), nt=nt, seed=100 * epi + i)
        if i < 4:
            w4.check_gemv(be, M, N, K, epi, norm=not ((i + epi) & 1), nt=nt, seed=100 * epi + i + 50)


def test_gemv_w4_reaches_every_instance(be):
    for (M, N, K, nt) in w4.GEMV_CASES:
        w4.check_gemv(be, M, N, K, 1, nt=nt)
    assert w4.instances_seen(be) == w4.W4_INSTANCES, sorted(w4.W4_INSTANCES - w4.instances_seen(be))


def test_gemv_w4_fp16_operands(be16):
    """v_cvt_scalef32_pk_f16_fp4 in the -DVC_F16 build"""
    w4.check_gemv(be16, 9, 80, 384, 0, norm=True, nt=2)
    w4.check_gemv(be16, 17, 16, 128, 2, nt=1)
    w4.check_gemv(be16, 32, 80, 1408, 3, norm=True, nt=4)


@pytest.mark.parametrize("epi,ksplit", [(0, 0), (1, 2), (3, 0), (2, 3)])
def test_gemv_w4_rows_agree(be, epi, ksplit):
    w4.check_rows_agree(be, 80, 1408 if ksplit != 2 else 384, epi, norm=epi != 2, ksplit=ksplit, nts=(1, 2, 4), seed=epi)


@pytest.mark.parametrize("M,epi", [(6, 1), (8, 2), (13, 0), (16, 3), (3, 2)])
def test_gemv_w4_split(be, M, epi):
    w4.check_gemv_split(be, M, 80, 384, epi, seed=M)


# the decoder linears of the 7b and 13b models: (N, K, epilogue)
TRUE_SHAPES = [(12288, 4096, 0), (4096, 4096, 2), (22016, 4096, 3), (4096, 11008, 2),
               (15360, 5120, 0), (5120, 5120, 2), (27648, 5120, 3), (5120, 13824, 2)]


@pytest.mark.parametrize("N,K,epi", TRUE_SHAPES)
def test_gemv_w4_true_shapes(be, N, K, epi):
    w4.check_true_shape(be, N, K, epi, seed=N % 97)


@pytest.mark.parametrize("name", ["ds_img_depth_seg", "vc_img_seg"])
def test_w4_weight_format(name):
    print(name, w4.check_w4_weights(name, n_new=6))


def test_w4_weight_format_fp16_operand_library():
    print(w4.check_w4_weights("ds_img_depth_seg", n_new=6, split=False, operands="fp16"))


def test_w4_extend():
    w4.check_extend("ds_img_depth_seg", None, 5)


def test_w4_pooled_generate_keeps_the_ids():
    w4.check_pool(None)


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    d, name = w4.tiny_checkpoint(tmp_path_factory.mktemp("ckpt"))
    return w4.load_model(d, name)


def test_w4_load_pretrained_model_generates_the_engines_ids(model):
    w4.check_model_ids(model)


def test_w4_beam_search_device_loop_equals_host_loop(model):
    w4.check_beams(model)


def test_w4_refuses_hidden_size_not_divisible_by_128():
    w4.check_refused_hidden_size(None)
