"""Guard bands for the tests that call the C ABI on outputs of their own (tests/test_gpu_xf_edges.py, tests/test_gpu_gmm_edges.py,
tests/test_gpu_bin_edges.py, tests/test_gpu_update_edges.py): an fp32 (or, for bin indices, int64) output inside a sentinel-filled
buffer.  No word outside the output may change, none inside may keep the sentinel.  _FencedBig (tests/test_gpu_large_extent.py) is
the same for outputs past 2^31 words."""
import numpy as np
import torch

SENTINEL = 0x7FC0DEAD                   # a NaN with a payload: no arithmetic on finite inputs stores this word
PAD = 1024                              # words (4 KiB) of sentinel before and after every output


class _Fenced:
    """An fp32 output of `shape` in the middle of a sentinel-filled int32 buffer; dtype=torch.int64: two words per element
    (offset_words even), whose low and high words -- a small index and 0 -- are never the sentinel either."""

    def __init__(self, what, *shape, offset_words=0, dtype=torch.float32):
        wpe = {torch.float32: 1, torch.int64: 2}[dtype]
        assert offset_words % wpe == 0
        self.what, self.n = what, int(np.prod(shape)) * wpe
        self.buf = torch.full((PAD + offset_words + self.n + PAD,), SENTINEL, dtype=torch.int32, device="cuda")
        self.words = self.buf[PAD + offset_words:PAD + offset_words + self.n]
        self.t = self.words.view(dtype).view(*shape)
        assert self.t.data_ptr() % 16 == 4 * (offset_words % 4)

    def ptr(self):
        return self.t.data_ptr()

    def untouched(self):
        return bool((self.buf == SENTINEL).all())

    def check(self):
        lo, hi = self.buf[:self.words.storage_offset()], self.buf[self.words.storage_offset() + self.n:]
        assert lo.numel() >= PAD and hi.numel() >= PAD
        assert bool((lo == SENTINEL).all()) and bool((hi == SENTINEL).all()), f"{self.what}: a word outside the output was written"
        assert not bool((self.words == SENTINEL).any()), f"{self.what}: an output word was never written"
        return self.t


SCAN = 1 << 26                          # words per fill / scan call of _FencedBig


class _FencedBig(_Fenced):
    """_Fenced for outputs past 2^31 words (tests/test_gpu_large_extent.py): the sentinel fill and the scans run over slices of SCAN
    words, so that torch itself is never asked for a 2^31-element fill or reduction.  dtype=torch.uint8: four bytes per word
    (the element count a multiple of 4), whose 0 / 1 bytes never form the sentinel."""

    def __init__(self, what, *shape, offset_words=0, dtype=torch.float32):
        n_el = int(np.prod(shape))
        if dtype == torch.uint8:
            assert n_el % 4 == 0
            self.n = n_el // 4
        else:
            assert dtype == torch.float32
            self.n = n_el
        self.what = what
        self.buf = torch.empty((PAD + offset_words + self.n + PAD,), dtype=torch.int32, device="cuda")
        for a in range(0, self.buf.numel(), SCAN):
            self.buf[a:a + SCAN].fill_(SENTINEL)
        self.words = self.buf[PAD + offset_words:PAD + offset_words + self.n]
        self.t = self.words.view(dtype).view(*shape)
        assert self.t.data_ptr() % 16 == 4 * (offset_words % 4)

    def _sentinels(self, words):
        count = torch.zeros((), dtype=torch.int64, device="cuda")
        for a in range(0, words.numel(), SCAN):
            count += (words[a:a + SCAN] == SENTINEL).sum()
        return int(count)

    def untouched(self):
        return self._sentinels(self.buf) == self.buf.numel()

    def check(self):
        lo, hi = self.buf[:self.words.storage_offset()], self.buf[self.words.storage_offset() + self.n:]
        assert lo.numel() >= PAD and hi.numel() >= PAD
        assert bool((lo == SENTINEL).all()) and bool((hi == SENTINEL).all()), f"{self.what}: a word outside the output was written"
        left = self._sentinels(self.words)
        assert left == 0, f"{self.what}: {left} output words were never written"
        return self.t
