"""CPU: the canonical oracle's distances equal torch's own CPU results bit for bit at latent widths 209 ... 512, for both
distance rules (LLFQ: torch.norm(z - e, dim=-1); plain VQVAE: (z - e).pow(2).sum(-1)) and for one and several threads.
The wide screened routes decide uncertified rows in the oracle's order; this pins that order to the reference's."""
import numpy as np
import pytest
import torch

from oracle import lipvq_oracle as O


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("dist", [O.DIST_NORM, O.DIST_SQSUM])
@pytest.mark.parametrize("D", [209, 256, 263, 264, 300, 384, 511, 512])
def test_oracle_distances_equal_torch_at_wide_latents(oracle, D, dist, threads):
    rng = np.random.default_rng(D * 7 + dist)
    z = rng.standard_normal((64, D)).astype(np.float32)
    cb = rng.standard_normal((128, D)).astype(np.float32)
    z[:16] = cb[:16] + np.float32(1e-3) * rng.standard_normal((16, D)).astype(np.float32)     # near pairs too
    ours = oracle.distances(z, cb, dist=dist)
    before = torch.get_num_threads()
    torch.set_num_threads(threads)
    try:
        diff = torch.from_numpy(z)[:, None, :] - torch.from_numpy(cb)[None, :, :]
        ref = torch.norm(diff, dim=-1) if dist == O.DIST_NORM else diff.pow(2).sum(-1)
    finally:
        torch.set_num_threads(before)
    assert np.array_equal(ours, ref.numpy())
