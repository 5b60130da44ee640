"""CPU: ``derived.stamp`` / ``derived.mark_written`` (the one parameter stamp and the one write notice) and the two pieces of
``capture`` that need no GPU: ``Snapshot``'s in-place restore and ``copy_in``'s checks.  The package is imported as
tests/test_cache_coherence_host.py imports it."""
import pytest
import torch


def _modules():
    import lipvq_vae_amd  # noqa: F401
    from lipvq_vae_amd import capture, derived
    return derived, capture


def _fields_changed(before, after):
    """Per tensor: the set of fields of its (data_ptr, _version) pair that differ."""
    assert len(before) == len(after)
    return [{name for name, x, y in zip(("data_ptr", "version"), b, a) if x != y} for b, a in zip(before, after)]


def test_stamp_is_one_address_version_pair_per_tensor():
    derived, _ = _modules()
    a, b = torch.nn.Parameter(torch.randn(3, 2)), torch.randn(5)
    s = derived.stamp(t for t in (a, b))                               # any iterable
    assert s == ((a.data_ptr(), a._version), (b.data_ptr(), b._version)) and derived.stamp((a, b)) == s
    assert derived.stamp(()) == ()


def test_stamp_sees_versions_and_addresses_and_nothing_else():
    derived, _ = _modules()
    a, b = torch.nn.Parameter(torch.randn(3, 2)), torch.nn.Parameter(torch.randn(4))
    s0 = derived.stamp((a, b))
    with torch.no_grad():
        a.mul_(2.0)                                                    # an in-place op: a's version, nothing else
    s1 = derived.stamp((a, b))
    assert _fields_changed(s0, s1) == [{"version"}, set()]
    derived.mark_written(t for t in (b,))                              # the write notice: b's version, nothing else
    s2 = derived.stamp((a, b))
    assert _fields_changed(s1, s2) == [set(), {"version"}] and s2[1][1] == s1[1][1] + 1
    keep = a.data                                                      # (keeps the old storage alive: the new one cannot reuse its address)
    a.data = a.detach().clone()                                        # a new storage: a's address, nothing else
    s3 = derived.stamp((a, b))
    assert _fields_changed(s2, s3) == [{"data_ptr"}, set()] and keep.data_ptr() == s2[0][0]
    before = a.detach().clone()
    a.data.add_(1.0)                                                   # the documented blind spot: the values moved ...
    assert not torch.equal(a.detach(), before)
    assert derived.stamp((a, b)) == s3                                 # ... and neither field did


def _trained(n_steps):
    """Two CPU parameters and a torch AdamW that has taken n_steps steps on them."""
    torch.manual_seed(3)
    params = [torch.nn.Parameter(torch.randn(4, 3)), torch.nn.Parameter(torch.randn(5))]
    opt = torch.optim.AdamW(params, lr=1e-2)
    _steps(params, opt, n_steps)
    return params, opt


def _steps(params, opt, n):
    for i in range(n):
        for p in params:
            p.grad = torch.full_like(p, 0.5 + i)
        opt.step()


def _state_tensors(params, opt):
    return [v for p in params for _, v in sorted(opt.state.get(p, {}).items()) if torch.is_tensor(v)]


@pytest.mark.parametrize("had_state", [False, True])
def test_snapshot_restores_in_place(had_state):
    _, capture = _modules()
    params, opt = _trained(2 if had_state else 0)
    lr = torch.tensor(1e-2)                                            # a tensor-valued lr travels with the parameters
    assert len(_state_tensors(params, opt)) == (6 if had_state else 0)
    want_params = [p.detach().clone() for p in params]
    want_state = [v.clone() for v in _state_tensors(params, opt)]
    snap = capture.Snapshot(params + [lr], opt, params)
    _steps(params, opt, 3)                                             # the "warm-up": real steps
    with torch.no_grad():
        lr.mul_(0.5)
    state = _state_tensors(params, opt)
    assert len(state) == 6 and all(not torch.equal(p.detach(), w) for p, w in zip(params, want_params))
    ptrs = [t.data_ptr() for t in params + [lr] + state]
    snap.restore()
    assert [t.data_ptr() for t in params + [lr] + _state_tensors(params, opt)] == ptrs       # nothing was replaced
    assert all(torch.equal(p.detach(), w) for p, w in zip(params, want_params)) and lr.item() == pytest.approx(1e-2, rel=1e-7)
    if had_state:                                                      # the values are back ...
        assert all(torch.equal(v, w) for v, w in zip(state, want_state))
        assert all(float(opt.state[p]["step"]) == 2.0 for p in params)
    else:                                                              # ... or the state the warm-up created is a fresh optimizer's
        assert all(not v.any() for v in state)


def test_copy_in_copies_or_raises_before_copying():
    _, capture = _modules()
    static = (torch.zeros(2, 3), torch.zeros(4))
    x, y = torch.randn(2, 3), torch.randn(4)
    ptrs = [s.data_ptr() for s in static]
    capture.copy_in(static, (x, y))
    assert torch.equal(static[0], x) and torch.equal(static[1], y) and [s.data_ptr() for s in static] == ptrs
    kept = [s.clone() for s in static]
    with pytest.raises(ValueError, match=r"graphed step was captured for 2 inputs, got 1"):
        capture.copy_in(static, (torch.ones(2, 3),))
    with pytest.raises(ValueError, match=r"graphed step was captured for 2 inputs, got 3"):
        capture.copy_in(static, (x, y, y))
    with pytest.raises(ValueError, match=r"graphed step was captured for \[\(2, 3\), \(4,\)\], got \(5,\)"):
        capture.copy_in(static, (torch.ones(2, 3), torch.ones(5)))    # the FIRST input fits: it must not have been copied
    assert all(torch.equal(s, k) for s, k in zip(static, kept))
    one = torch.zeros(2, 3)                                            # the single-tensor form and its wording
    capture.copy_in(one, x, "captured")
    assert torch.equal(one, x)
    with pytest.raises(ValueError, match=r"^captured for \(2, 3\), got \(3, 2\)$"):
        capture.copy_in(one, torch.ones(3, 2), "captured")
    with pytest.raises(ValueError, match=r"^graphed step was captured for \(2, 3\), got \(2, 4\)$"):
        capture.copy_in(one, torch.ones(2, 4))
    assert torch.equal(one, x)
