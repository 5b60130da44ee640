"""Plain-torch restatement of the policy's GMM output head (reference robomimic/models/obs_nets.py:763-771 -- the
ObservationDecoder's three Linears -- and robomimic/models/policy_nets.py:2545-2575 -- tanh, softplus + min_std, the Normal /
Independent / Categorical / MixtureSameFamily objects), as functions of a ``state_dict`` -- test infrastructure in the style of
tests/gpt_ref.py: it issues the reference's own ops (``F.linear``, ``torch.tanh``, ``F.softplus`` / ``torch.exp``, ``D.Normal``,
``D.Independent``, ``D.Categorical``, ``D.MixtureSameFamily``), runs on any device and in any float dtype (the float64 yardstick
of tests/test_gpu_gmm.py is this code on ``.double()`` tensors), and scripts/bench_gmm.py times it as the eager baseline.
The reference's own classes cannot be imported for this: obs_nets.py pulls in ``clip`` and Hugging Face ``transformers``.
"""
import math

import torch
import torch.distributions as D
import torch.nn.functional as F

LOW_NOISE_STD = 1e-4                      # policy_nets.py:2557
KEYS = ("nets.mean.weight", "nets.mean.bias", "nets.scale.weight", "nets.scale.bias", "nets.logits.weight", "nets.logits.bias")


def decoder(sd, feats, num_modes, ac_dim, prefix="nets."):
    """obs_nets.py:763-771 with the output shapes of policy_nets.py:2507-2516: the raw (mean [..., M, A], scale [..., M, A],
    logits [..., M]) of feats [..., E]."""
    lead = tuple(feats.shape[:-1])
    mean = F.linear(feats, sd[prefix + "mean.weight"], sd[prefix + "mean.bias"]).reshape(lead + (num_modes, ac_dim))
    scale = F.linear(feats, sd[prefix + "scale.weight"], sd[prefix + "scale.bias"]).reshape(lead + (num_modes, ac_dim))
    logits = F.linear(feats, sd[prefix + "logits.weight"], sd[prefix + "logits.bias"]).reshape(lead + (num_modes,))
    return mean, scale, logits


def activate(means, scales, min_std=0.01, std_activation="softplus", low_noise=False):
    """policy_nets.py:2549-2560 (use_tanh = False): (tanh(mean), scale)."""
    means = torch.tanh(means)
    if low_noise:
        scales = torch.ones_like(means) * LOW_NOISE_STD
    else:
        scales = {"softplus": F.softplus, "exp": torch.exp}[std_activation](scales) + min_std
    return means, scales


def mixture(means, scales, logits):
    """policy_nets.py:2564-2575 from activated means / scales and raw logits."""
    component = D.Independent(D.Normal(loc=means, scale=scales, validate_args=False), 1)
    return D.MixtureSameFamily(mixture_distribution=D.Categorical(logits=logits, validate_args=False), component_distribution=component,
                               validate_args=False)


def gmm_dist(sd, feats, num_modes, ac_dim, min_std=0.01, std_activation="softplus", low_noise=False):
    """The distribution forward_train returns, from the head's state_dict and feats [..., E]."""
    means, scales, logits = decoder(sd, feats, num_modes, ac_dim)
    means, scales = activate(means, scales, min_std, std_activation, low_noise)
    return mixture(means, scales, logits)


def gmm_log_prob(sd, feats, actions, num_modes, ac_dim, min_std=0.01, std_activation="softplus", low_noise=False):
    return gmm_dist(sd, feats, num_modes, ac_dim, min_std, std_activation, low_noise).log_prob(actions)


def log_prob_by_hand(means, scales, logits, actions):
    """logsumexp_m(log_softmax(logits)_m + sum_a [-(x - mu)^2 / (2 sigma^2) - log sigma - log(2 pi) / 2]) written out, from
    activated means / scales [..., M, A], raw logits [..., M] and actions [..., A]."""
    x = actions.unsqueeze(-2)
    ell = (-(x - means) ** 2 / (2.0 * scales ** 2) - torch.log(scales) - 0.5 * math.log(2.0 * math.pi)).sum(-1)
    logpi = logits - torch.logsumexp(logits, -1, keepdim=True)
    return torch.logsumexp(logpi + ell, -1), ell, logpi


def closed_form_grads(pre_mean, pre_scale, logits, actions, g, min_std=0.01, std_activation="softplus"):
    """The gradients of sum(g * log_prob) with respect to the three pre-activations, in closed form (responsibilities
    r = softmax(log pi + l)): g (r - pi);  g r (x - mu) / sigma^2 (1 - mu^2);  g r ((x - mu)^2 / sigma^3 - 1 / sigma) sigma'."""
    mu, sg = activate(pre_mean, pre_scale, min_std, std_activation)
    _, ell, logpi = log_prob_by_hand(mu, sg, logits, actions)
    r = torch.softmax(logpi + ell, -1)
    if std_activation == "softplus":
        dsg = torch.where(pre_scale > 20.0, torch.ones_like(pre_scale), torch.sigmoid(pre_scale))
    else:
        dsg = torch.exp(pre_scale)
    d = actions.unsqueeze(-2) - mu
    gr = (g.unsqueeze(-1) * r).unsqueeze(-1)
    return gr * d / sg ** 2 * (1.0 - mu ** 2), gr * (d ** 2 / sg ** 3 - 1.0 / sg) * dsg, g.unsqueeze(-1) * (r - logpi.exp())


def sample_by_inverse_cdf(sd, feats, u, eps, num_modes, ac_dim, min_std=0.01, std_activation="softplus", low_noise=False):
    """The sampler of GMMActionHead.forward in the dtype of its inputs: row n takes the first mode m with u[n] < sum_{j <= m}
    softmax(logits)_j (the last if none), action = mu_m + sigma_m eps.  Returns (actions [..., A], modes [...], margin [...]) with
    margin = the distance of u from the nearest interior CDF boundary (inf for one mode)."""
    means, scales, logits = decoder(sd, feats, num_modes, ac_dim)
    means, scales = activate(means, scales, min_std, std_activation, low_noise)
    cdf = torch.softmax(logits, -1).cumsum(-1)
    modes = (u.unsqueeze(-1) >= cdf).sum(-1).clamp(max=num_modes - 1)
    idx = modes[..., None, None].expand(modes.shape + (1, ac_dim))
    mu, sg = means.gather(-2, idx).squeeze(-2), scales.gather(-2, idx).squeeze(-2)
    if num_modes > 1:
        margin = (u.unsqueeze(-1) - cdf[..., :-1]).abs().min(-1).values
    else:
        margin = torch.full_like(u, float("inf"))
    return mu + sg * eps, modes, margin
