"""Derived state (packed weights, the prepared codebook, code tables, a prompt's keys and values, a forward's saved tensors) and the
tensors under it: the one definition of "this tensor changed" (``stamp``) and of "I wrote it behind autograd's back" (``mark_written``)."""
import torch


def stamp(tensors) -> tuple:
    """One ``(data_ptr, _version)`` pair per tensor: the key of every consumer of derived state.  It sees what bumps
    ``Tensor._version`` (an in-place torch op: an optimizer step, ``load_state_dict``; ``mark_written``) and what moves the storage
    (``p.data = new``, ``load_state_dict(assign=True)``, ``.to()`` / ``.cuda()`` / ``.float()``: they keep the version, not the address).
    What it CANNOT see: writes that bypass autograd's version counter -- ``p.data.add_(..)`` (the reference's own
    ``embedding.weight.data.uniform_()`` idiom), a captured optimizer step replayed from a HIP graph, a raw-pointer writer -- unless
    the writer calls ``mark_written``.  After such a write call ``invalidate_caches()``, ``prefill()`` / ``set_prompt()`` yourself."""
    return tuple((t.data_ptr(), t._version) for t in tensors)


def mark_written(tensors) -> None:
    """Bump each tensor's version, as an in-place torch op would: what a raw-pointer or replayed-graph writer owes every ``stamp``."""
    for t in tensors:
        torch.autograd.graph.increment_version(t)


class _PackCache:
    """Re-lays weights out for the MFMA kernels only when ``stamp`` of the tensors, or a device, changed.  After a write it cannot see
    call ``module.invalidate_caches()``; ``load_state_dict``, ``_apply`` (``.to()``, ``.cuda()``) and ``train()`` / ``eval()`` do."""
    _key = _val = None               # (an empty cache)

    def get(self, tensors, build):
        key = (stamp(tensors), tuple(t.device for t in tensors))
        if key != self._key:
            self._key, self._val = key, build()
        return self._val

    def invalidate(self):
        self._key = self._val = None

    def __deepcopy__(self, memo):
        return type(self)()          # a copied module builds its own: the key holds the ORIGINAL's addresses
