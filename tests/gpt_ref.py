"""Plain-torch restatement of the transformer backbone's op sequence (reference robomimic/models/transformers.py:153-206,
:296-302, :436-440), as functions of a ``state_dict`` -- test infrastructure in the style of tests/backward_ref.py: it runs on
any device and in any float dtype (the float64 evaluations of tests/test_gpu_gpt.py are this code on ``.double()`` tensors),
and scripts/bench_gpt.py times it as the eager baseline.

With fp32 CPU tensors it issues the SAME torch ops in the same order as the reference module (``nn.Linear`` is ``F.linear``,
``nn.LayerNorm`` is ``F.layer_norm``, ``nn.GELU`` is ``F.gelu``), so it reproduces the fixtures' fp32 outputs and gradients
bit for bit (tests/test_gpt_host.py uses ``torch.equal``).  The optional ``keep`` masks restate dropout with a GIVEN mask
(``x * keep / keep_prob``), which is what the kernels take; torch's own dropout draws its mask internally and cannot be
compared in bits.
"""
import math

import torch
import torch.nn.functional as F


def attention_ref(qkv, num_heads, mask=None, keep=None, keep_prob=1.0):
    """qkv [B, T, 3E] -> [B, T, E] (transformers.py:174-201).  mask [1, 1, >=T, >=T] (0 = closed) or None; keep [B, H, T, T] or None."""
    B, T, E3 = qkv.shape
    D = E3 // 3
    DH = D // num_heads
    q, k, v = torch.chunk(qkv, 3, dim=-1)
    k = k.view(B, T, num_heads, DH).transpose(1, 2)
    q = q.view(B, T, num_heads, DH).transpose(1, 2)
    v = v.view(B, T, num_heads, DH).transpose(1, 2)
    att = (q @ k.transpose(-2, -1)) * (1.0 / math.sqrt(k.size(-1)))
    if mask is not None:
        att = att.masked_fill(mask[..., :T, :T] == 0, float("-inf"))
    att = F.softmax(att, dim=-1)
    if keep is not None:
        att = att * keep.to(att.dtype) / keep_prob
    y = att @ v
    return y.transpose(1, 2).contiguous().view(B, T, D)


def causal_mask(T, causal=True, device=None):
    m = torch.ones(T, T, device=device)
    return (torch.tril(m) if causal else m).view(1, 1, T, T)


def block_forward(sd, prefix, x, num_heads, keeps=None, keep_prob=(1.0, 1.0, 1.0), p_out=0.0):
    """One SelfAttentionBlock (transformers.py:296-302).  keeps = (attention [B,H,T,T], attention output [B,T,E], mlp output [B,T,E])
    masks or None; p_out > 0 applies torch's own F.dropout to the two block outputs instead (what the reference's nn.Dropout does)."""
    E = x.shape[-1]
    ka, ko, km = keeps if keeps is not None else (None, None, None)
    y = F.layer_norm(x, (E,), sd[prefix + "ln1.weight"], sd[prefix + "ln1.bias"], 1e-5)
    qkv = F.linear(y, sd[prefix + "attention.nets.qkv.weight"])
    y = attention_ref(qkv, num_heads, sd[prefix + "attention.mask"], ka, keep_prob[0])
    y = F.linear(y, sd[prefix + "attention.nets.output.weight"], sd[prefix + "attention.nets.output.bias"])
    if ko is not None:
        y = y * ko.to(y.dtype) / keep_prob[1]
    if p_out > 0.0:
        y = F.dropout(y, p_out, True)
    x = x + y
    y = F.layer_norm(x, (E,), sd[prefix + "ln2.weight"], sd[prefix + "ln2.bias"], 1e-5)
    y = F.linear(y, sd[prefix + "mlp.0.weight"], sd[prefix + "mlp.0.bias"])
    y = F.gelu(y)
    y = F.linear(y, sd[prefix + "mlp.2.weight"], sd[prefix + "mlp.2.bias"])
    if km is not None:
        y = y * km.to(y.dtype) / keep_prob[2]
    if p_out > 0.0:
        y = F.dropout(y, p_out, True)
    return x + y


def gpt_forward(sd, inputs, num_layers, num_heads):
    """GPT_Backbone.forward in eval mode (transformers.py:436-440) from its state_dict."""
    x = inputs
    for i in range(num_layers):
        x = block_forward(sd, f"nets.transformer.{i}.nets.", x, num_heads)
    return F.layer_norm(x, (x.shape[-1],), sd["nets.output_ln.weight"], sd["nets.output_ln.bias"], 1e-5)


def objective_weights(seed, shape):
    """The fixed tensor r of the fixtures' scalar objective L = sum(out * r)."""
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed + 2))


def state_hash(sd):
    """sha256 over (key, bytes) of a state_dict in its own order."""
    import hashlib
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(v.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


# the parameter gradients a fixture keeps (small ones from the first block, the last block and the head; `{last}` = num_layers - 1)
STORED_PARAM_GRADS = ("nets.output_ln.weight", "nets.output_ln.bias", "nets.transformer.0.nets.ln1.weight",
                      "nets.transformer.0.nets.ln2.bias", "nets.transformer.0.nets.mlp.2.bias",
                      "nets.transformer.0.nets.mlp.0.bias", "nets.transformer.{last}.nets.attention.nets.output.bias")
# and the first rows of two weight matrices of the first block
STORED_WEIGHT_ROWS = (("nets.transformer.0.nets.attention.nets.qkv.weight", 4), ("nets.transformer.0.nets.mlp.0.weight", 4))
