"""The pieces of every HIP-graph capture here (``nnfn.GraphedEval``, ``icl.GraphedTokenizerStep``, ``icl.GraphedPolicyStep``), once each;
the ORDER they are called in is each caller's safety argument (see the class docstrings in icl.py) and stays with the caller."""
import torch


def warm_up(fn, n: int, device=None) -> None:
    """``fn()`` n times on a side stream of ``device`` that waits for the current stream and is waited for by it: first-use work
    (LDS reservations, lazy module and optimizer state, workspaces) is issued here, not while capturing."""
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        for _ in range(n):
            fn()
    torch.cuda.current_stream(device).wait_stream(side)


class Snapshot:
    """Values of ``tensors`` (parameters, module buffers, tensor-valued ``lr``s) and of the ``optimizer``'s state for the parameters
    ``owned``, as they are now; ``restore()`` puts them back.  The warm-up steps of a graphed training step are REAL steps (they
    have to be: they make the one-time work happen), but construction must not train the model: what a step writes is put back IN
    PLACE after them -- in place, because the capture that follows records these tensors' addresses and must find them allocated:
    state the warm-up created is zeroed (= a fresh optimizer), state from before gets its values back.  Replay k = eager step k."""

    def __init__(self, tensors, optimizer, owned):
        self._optimizer, self._saved = optimizer, [(t, t.detach().clone()) for t in tensors]
        self._state = [(p, {k: v.detach().clone() for k, v in optimizer.state.get(p, {}).items() if torch.is_tensor(v)}) for p in owned]

    @torch.no_grad()
    def restore(self) -> None:
        for t, s in self._saved:
            t.copy_(s)
        for p, old in self._state:
            for k, v in self._optimizer.state.get(p, {}).items():
                if torch.is_tensor(v):
                    v.copy_(old[k]) if k in old else v.zero_()


def capture(fn):
    """(graph, fn()) with ``fn`` recorded into a new HIP graph; its result is the graph's static output, refilled by every replay."""
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        return graph, fn()


def copy_in(static, inputs, what: str = "graphed step was captured") -> None:
    """Copy ``inputs`` into the ``static`` buffers of a capture (one tensor each, or two sequences); ``ValueError``, before anything
    is copied, when the number of inputs or a shape is not the captured one."""
    single = isinstance(static, torch.Tensor)
    statics, inputs = ((static,), (inputs,)) if single else (static, inputs)
    if len(inputs) != len(statics):
        raise ValueError(f"{what} for {len(statics)} inputs, got {len(inputs)}")
    for x, s in zip(inputs, statics):
        if x.shape != s.shape:
            raise ValueError(f"{what} for {tuple(static.shape) if single else [tuple(t.shape) for t in statics]}, got {tuple(x.shape)}")
    for x, s in zip(inputs, statics):
        s.copy_(x)
