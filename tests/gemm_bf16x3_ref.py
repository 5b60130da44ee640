"""CPU references of the bf16x3 Linear tests (tests/test_gemm_bf16x3_host.py, tests/test_gpu_gemm_bf16x3.py): the split of an
fp32 operand into two bf16 numbers as include/lipvq.h states it, the float64 three-term product of the split operands with
its magnitude sum, the exact product, and the bounds.  Pure torch on the CPU, no torch.cuda.  Shapes, inputs and layouts are
those of tests/gemm_bf16_cases.py (NT forward, NN input gradient, TN weight gradient; a LINE of an operand feeds one row (A)
or one column (B) of the result).

    split:    hi = bf16_rne(v),  lo = bf16_rne(v - float(hi))  (the subtraction is exact in fp32; lo = 0 where hi is not finite)
    product:  s3 = sum_k (a_lo b_hi + a_hi b_lo + a_hi b_hi),   R3 = sum_k (|a_lo b_hi| + |a_hi b_lo| + |a_hi b_hi|)
    bounds:   |got - s3|   <= 2 (3 L + 1) 2^-24 R3                     twice any-order round-to-nearest over the 3 L terms
              |s3 - exact| <= 3 2^-16 (1 + 2^-7) R_exact               the two residuals and the dropped a_lo b_lo term
              |got - exact| <= the sum of the two                      ("the combined bound")
"""
from __future__ import annotations

import torch

import gemm_bf16_cases as C

EPS = C.EPS
SPLIT_REL = 3 * 2.0 ** -16 * (1 + 2.0 ** -7)          # per product, operands 0 or normal, no bf16 overflow
WITNESS_VALUE = 1.0 + 2.0 ** -9                       # hi = 1, lo = 2^-9 exactly

NS = (1, 33, 130, 240)                                # the shapes of tests/test_gpu_gemm_bf16.py
KJ = ((16, 8), (72, 24), (512, 136), (2048, 512))
LAYOUTS = ("NT", "NN", "TN")


def split(t):
    """(hi, lo) of an fp32 tensor, as float64.  Asserts that t - hi is exact in fp32 wherever hi is finite."""
    assert t.dtype == torch.float32
    hi = t.bfloat16().float()
    fin = torch.isfinite(hi)
    d = torch.where(fin, t - hi, torch.zeros_like(t))
    exact = torch.where(fin, t.double() - hi.double(), torch.zeros_like(t, dtype=torch.float64))
    assert torch.equal(d.double(), exact), "t - bf16(t) is not exact in fp32"
    lo = d.bfloat16().float()
    return hi.double(), lo.double()


def _mm(layout, A, B):
    if layout == "NT":
        return A @ B.t()
    if layout == "NN":
        return A @ B
    return A.t() @ B


def product3(layout, A, B):
    """(s3, R3) in float64 from the split operands; IEEE specials propagate as IEEE says."""
    ah, al = split(A)
    bh, bl = split(B)
    s3 = _mm(layout, al, bh) + _mm(layout, ah, bl) + _mm(layout, ah, bh)
    R3 = _mm(layout, al.abs(), bh.abs()) + _mm(layout, ah.abs(), bl.abs()) + _mm(layout, ah.abs(), bh.abs())
    return s3, R3


def product_exact(layout, A, B):
    """(exact, R_exact): the float64 product of the unrounded operands and sum |a b|."""
    return _mm(layout, A.double(), B.double()), _mm(layout, A.double().abs(), B.double().abs())


def concat_fp32(layout, A, B):
    """The fp32 CPU product of the reduction-concatenated operands [a_lo | a_hi | a_hi] . [b_hi | b_lo | b_hi]: the three-term
    product as ONE fp32 matrix product of three times the reduction length (every factor is a bf16 number, so every product
    is exact in fp32 and only the accumulation rounds)."""
    ah, al = (t.float() for t in split(A))
    bh, bl = (t.float() for t in split(B))
    ra = {"NT": 1, "NN": 1, "TN": 0}[layout]                  # the reduction axis of A and of B as stored
    rb_ = {"NT": 1, "NN": 0, "TN": 0}[layout]
    return _mm(layout, torch.cat([al, ah, ah], ra), torch.cat([bh, bl, bh], rb_))


def combined_bound(L, R_exact, R3):
    return SPLIT_REL * R_exact + 2 * (3 * L + 1) * EPS * R3


_refs = {}


def ref(layout, N, K, J):
    """dict(A, B, L, s3, R3, exact, R_exact, plain) of one shape and layout, computed once and never modified; plain is the
    float64 product of the bf16-ROUNDED operands (what the "bf16" mode computes, without its accumulation error)."""
    key = (layout, N, K, J)
    if key not in _refs:
        c = C.case(N, K, J)
        A, B, _, _ = C.operands(layout, c["x"], c["W"], c["g"])
        r = dict(A=A, B=B, L=C.launch_dims(layout, N, K, J)[2])
        r["s3"], r["R3"] = product3(layout, A, B)
        r["exact"], r["R_exact"] = product_exact(layout, A, B)
        r["plain"] = C.product64(layout, A, B)[0]
        _refs[key] = r
    return _refs[key]


def all_cases():
    """(layout, N, K, J) of every product the GPU test runs: NS x KJ in all three layouts and every INSTANCES row."""
    out = [(lay, N, K, J) for lay in LAYOUTS for N in NS for K, J in KJ]
    out += [(i.layout, i.N, i.K, i.J) for i in C.INSTANCES]
    return out


def case_id(case):
    return "{}-{}x{}x{}".format(*case)


def witness_operands(layout, N, K, J, fill_a, fill_b):
    """(x, W, g) with the layout's A and B operands constant: 1 + 2^-9 where filled, else 1; the third tensor is ones."""
    a = torch.full((1,), WITNESS_VALUE if fill_a else 1.0)
    b = torch.full((1,), WITNESS_VALUE if fill_b else 1.0)
    x, W, g = torch.ones(N, K), torch.ones(J, K), torch.ones(N, J)
    if layout == "NT":
        x, W = x * a, W * b
    elif layout == "NN":
        g, W = g * a, W * b
    else:
        g, x = g * a, x * b
    return x, W, g


def witness_value(L, fill_a, fill_b):
    """The exact result element: L (1 + 2^-8) with both operands filled (hi hi = 1, each cross term 2^-9, lo lo dropped),
    L (1 + 2^-9) with one.  Every partial sum is a multiple of 2^-9 below 2^15: exact in fp32 in any order."""
    assert L * (1 + 2.0 ** -8) < 2 ** 15
    return L * (1.0 + (2.0 ** -9) * (int(fill_a) + int(fill_b)))
