"""CPU: the host side of the backbone's bf16 matrix-pipe mode -- the GPTBackbone switch, the argument checks of the four new
entry points (sizes are checked before pointers, so null pointers do on a host without a GPU) and the row-chunk rule of the
weight gradient as include/lipvq.h states it."""
import pytest


def test_backbone_switch_round_trips_and_stays_out_of_the_state_dict():
    from lipvq_vae_amd.gpt import GPTBackbone
    net = GPTBackbone(64, 12, num_layers=1, num_heads=4)
    keys = list(net.state_dict().keys())
    assert net.matmul_precision == "fp32"
    assert net.set_matmul_precision("bf16") is net and net.matmul_precision == "bf16"
    assert list(net.state_dict().keys()) == keys
    with pytest.raises(ValueError, match="fp16"):
        net.set_matmul_precision("fp16")
    assert net.matmul_precision == "bf16"                                     # a refused value changes nothing
    assert net.set_matmul_precision("fp32").matmul_precision == "fp32"
    with pytest.raises(AttributeError):
        net.matmul_precision = "bf16"                                         # read-only: set_matmul_precision validates


def test_library_limits_are_reported_without_a_gpu():
    from lipvq_vae_amd import _capi
    lib = _capi.lib

    def fwd(N, K, J):
        return lib.lipvq_linear_act_bf16(None, None, None, None, None, N, K, J, 0, None)

    def nn(N, J, K):
        return lib.lipvq_linear_nn_bf16(None, None, None, N, J, K, None)

    def wg(N, J, K):
        return lib.lipvq_wgrad_bf16(None, None, None, None, None, N, J, K, None)

    for call in (fwd, nn, wg):
        assert call(240, 12, 64) == -2 and b"multiples of 8" in lib.lipvq_last_error()
        assert call(240, 64, 12) == -2 and b"multiples of 8" in lib.lipvq_last_error()
        assert call(0, 64, 64) == 0                                           # zero rows: no-op
        assert call(-1, 64, 64) == -1 and call(4, 0, 64) == -1
        assert call(240, 64, 64) == -1 and b"null" in lib.lipvq_last_error()  # limits pass, then the pointers
    assert lib.lipvq_linear_act_bf16(None, None, None, None, None, 4, 64, 64, 7, None) == -1     # not an activation


def _chunk(N, J, K):
    """The rule as include/lipvq.h writes it."""
    ceil = lambda a, b: -(-a // b)
    want = max(1, 1024 // (ceil(J, 128) * ceil(K, 128)))
    return max(64, 32 * ceil(ceil(N, want), 32))


def test_wgrad_workspace_follows_the_header_formula():
    from lipvq_vae_amd import _capi
    ws = _capi.lib.lipvq_wgrad_bf16_workspace_bytes
    assert _chunk(240, 512, 512) == 64 and ws(240, 512, 512) == 4 * (512 * 512 + 512) * 4
    assert _chunk(122880, 2048, 512) == 7680 and ws(122880, 2048, 512) == 16 * (2048 * 512 + 2048) * 4
    for N, J, K in ((1, 8, 16), (4100, 64, 64), (122880, 512, 512), (70000, 136, 2048)):
        assert ws(N, J, K) == -(-N // _chunk(N, J, K)) * (J * K + J) * 4, (N, J, K)
    assert ws(4100, 64, 64) == 65 * (64 * 64 + 64) * 4                       # 64 whole chunks and a ragged one of 4 rows
    assert ws(0, 64, 64) == 0 and ws(-3, 64, 64) == 0                         # (all answered with no device to ask)
