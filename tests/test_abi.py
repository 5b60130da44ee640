"""CPU: the C-ABI shared library loads and exports every symbol include/lipvq.h declares, and the
ctypes table (lipvq-vae_amd/_capi.py) covers exactly that set.  No compute calls (no GPU here)."""
import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def _declared():
    text = (ROOT / "include" / "lipvq.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(lipvq_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_the_path():
    names = _declared()
    for must in ("lipvq_mlp3_f32", "lipvq_nearest_f32", "lipvq_lipschitz_scale_f32", "lipvq_mse_pair_f32",
                 "lipvq_mlp3_bwd_f32", "lipvq_wgrad_f32", "lipvq_scatter_add_f32", "lipvq_lipschitz_bwd_f32"):
        assert must in names


def test_library_exports_every_declared_symbol():
    so = ROOT / "lipvq-vae_amd" / "_lipvq_hip.so"
    assert so.exists(), "build the HIP library first (__graft_entry__.build())"
    import torch  # noqa: F401  (maps torch's libamdhip64 first, as the product does)
    lib = ctypes.CDLL(str(so))
    for name in _declared():
        assert hasattr(lib, name), f"{name} declared in include/lipvq.h but not exported"
    lib.lipvq_abi_version.restype = ctypes.c_int
    assert lib.lipvq_abi_version() == 1


def test_ctypes_table_matches_header():
    import lipvq_vae_amd
    from lipvq_vae_amd import _capi
    assert sorted(_capi.SIGNATURES) == _declared()
    # retired with the default branch's own LayerNorm kernels (it runs the lipvq_gpt_layernorm_* entry points)
    for gone in ("lipvq_add_layernorm_f32", "lipvq_layernorm_bwd_f32"):
        assert gone not in _capi.SIGNATURES and not hasattr(_capi.lib, gone)
    # pure host-side entry points are callable without a GPU
    assert _capi.lib.lipvq_mlp3_packed_floats(7, 64, 128, 64) == (2 * 4 * 64 + 64) + (4 * 32 * 64 + 128) + (2 * 64 * 64 + 64)
    assert _capi.lib.lipvq_mse_workspace_bytes() > 0
    # one partial slab per chunk of rows: 64-row chunks below 16 384 rows, 1024-row chunks from 262 144 rows on
    assert _capi.lib.lipvq_wgrad_workspace_bytes(5000, 128, 64) == 79 * (128 * 64 + 128) * 4
    assert _capi.lib.lipvq_wgrad_workspace_bytes(300000, 128, 64) == 293 * (128 * 64 + 128) * 4


# lipvq_nearest_workspace_bytes(N) / lipvq_tokenize_workspace_bytes(N, D) as the library answered before the workspace layout
# moved into one struct (LqWorkspace, lipvq_screen.h): recorded from that build, not computed here from the same formula
_NEAREST_WS_BYTES = {1: 4416, 15: 5312, 16: 5376, 17: 5632, 80: 10240, 4096: 315456, 32768: 2494528, 524288: 39850048}
_TOKENIZE_WS_BYTES = {      # N: bytes at D = 7, 32, 64, 128, 208, 512
    1: (4700, 4800, 4928, 5184, 120192, 268864),
    15: (5988, 7488, 9408, 13248, 132736, 298432),
    16: (6080, 7680, 9728, 13824, 133632, 300544),
    17: (6364, 8064, 10240, 14592, 134720, 302848),
    80: (12736, 20736, 30976, 51456, 191744, 436480),
    4096: (430400, 840000, 1364288, 2412864, 3838272, 8966464),
    32768: (3412288, 6689088, 10883392, 19272000, 29872448, 69865792),
    524288: (54530368, 106959168, 174068032, 308285760, 476172608, 1113854272),
}


def test_workspace_sizes_are_the_recorded_ones():
    import lipvq_vae_amd
    from lipvq_vae_amd import _capi
    for N, want in _NEAREST_WS_BYTES.items():
        assert _capi.lib.lipvq_nearest_workspace_bytes(N) == want, N
    for N, row in _TOKENIZE_WS_BYTES.items():
        for D, want in zip((7, 32, 64, 128, 208, 512), row):
            assert _capi.lib.lipvq_tokenize_workspace_bytes(N, D) == want, (N, D)
    assert _capi.lib.lipvq_nearest_workspace_bytes(0) == 0 and _capi.lib.lipvq_tokenize_workspace_bytes(0, 64) == 0
    assert _capi.lib.lipvq_tokenize_workspace_bytes(16, 0) == 0


def test_missing_library_fails_loudly(tmp_path, monkeypatch):
    """The product must not fall back to anything when the extension is absent."""
    import importlib.util
    src = (ROOT / "lipvq-vae_amd" / "_capi.py").read_text()
    (tmp_path / "_capi.py").write_text(src)
    spec = importlib.util.spec_from_file_location("capi_copy", tmp_path / "_capi.py")
    mod = importlib.util.module_from_spec(spec)
    with pytest.raises(ImportError, match="no CPU fallback"):
        spec.loader.exec_module(mod)
