"""Host -> HBM batch staging: pinned double buffers + a copy stream, so the H2D transfer of batch i+1 overlaps the
training step of batch i.

The reference moves every batch with a synchronous ``.cuda()`` on the compute stream
(Train/temporal_transformer_shanghaitech.py:115-118): 805 MB per step at the headline LTN shape = 12.8 ms at PCIe Gen5
x16 (63 GB/s) in front of every step.  Here the loader thread's tensors are copied into two pinned host slabs and sent
with ``non_blocking=True`` on a side HIP stream; the compute stream only waits on the copy's event.
torch is used purely for memory/stream plumbing."""
from __future__ import annotations

import numpy as np
import torch


class PinnedFeeder:
    def __init__(self, batches, device, depth: int = 2):
        """``batches``: iterable of tuples of CPU tensors (the DataLoader contract: norm_feats, norm_labs, abnorm_feats,
        abnorm_labs).  Yields the same tuples as device tensors."""
        self.batches, self.device, self.depth = batches, torch.device(device), depth
        self.copy_stream = torch.cuda.Stream(device=self.device)
        self._slabs = [None] * depth          # pinned host buffers, reused
        self._dev = [None] * depth            # device buffers, reused (the step must finish before slot reuse)
        self._ready = [None] * depth          # copy-done events
        self._consumed = [None] * depth       # compute-done events (protect device buffer reuse)

    def _stage(self, slot, batch):
        if self._slabs[slot] is None or any(s.shape != b.shape or s.dtype != b.dtype for s, b in zip(self._slabs[slot], batch)):
            self._slabs[slot] = [torch.empty(b.shape, dtype=b.dtype).pin_memory() for b in batch]
            self._dev[slot] = [torch.empty(b.shape, dtype=b.dtype, device=self.device) for b in batch]
        if self._ready[slot] is not None:
            self._ready[slot].synchronize()            # previous H2D from this pinned slab has completed
        for s, b in zip(self._slabs[slot], batch):
            s.copy_(b)                                  # pageable -> pinned (host memcpy)
        with torch.cuda.stream(self.copy_stream):
            if self._consumed[slot] is not None:
                self.copy_stream.wait_event(self._consumed[slot])   # the step that read this device slot is done
            for d, s in zip(self._dev[slot], self._slabs[slot]):
                d.copy_(s, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.copy_stream)
        self._ready[slot] = ev

    def __iter__(self):
        it = iter(self.batches)
        pending = []
        slot = 0
        for _ in range(self.depth - 1):
            b = next(it, None)
            if b is None:
                break
            self._stage(slot, b)
            pending.append(slot)
            slot = (slot + 1) % self.depth
        while pending:
            b = next(it, None)
            if b is not None:
                self._stage(slot, b)
                pending.append(slot)
                slot = (slot + 1) % self.depth
            cur = pending.pop(0)
            torch.cuda.current_stream(self.device).wait_event(self._ready[cur])
            yield tuple(self._dev[cur])
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
            self._consumed[cur] = ev


class LazyRows:
    """``bank[idx]`` that has NOT been formed: one half (``kind`` 0 = normal, 1 = abnormal videos) of a training batch
    ``[2, bs, rows]`` of clip indices into an HBM-resident bank ``[clips, P, d]``.  ``engine.TrainStep`` hands the index vector to
    the fused gather + CLS-concat kernel (lstc_cls_concat_gather_fwd: the gathered batch is never written); everything else calls
    ``materialize()`` (lstc_gather_rows) and sees the ordinary ``[bs, rows, P, d]`` tensor."""

    def __init__(self, bank, idx_flat, kind, bs, rows, uniq=None, inverse=None, n_unique=0, slot_order=None):
        self.bank, self.idx_flat, self.kind, self.bs, self.rows = bank, idx_flat, kind, bs, rows
        self.shape = (bs, rows) + tuple(bank.shape[1:])
        self.device = bank.device
        # the batch's clips without their repeats (overlapping windows of short videos): ``uniq[:n_unique]`` the sorted distinct
        # clip indices, ``inverse[i]`` the place of clip ``idx_flat[i]`` among them (both int64, beside the indices); the host knows
        # ``n_unique`` before anything is launched.  Layer 0 projects the distinct rows only (functional.DedupRows).
        self.uniq, self.inverse, self.n_unique = uniq, inverse, int(n_unique)
        # ``slot_order``: the stable argsort of ``inverse`` (int64, from the host beside it; sorted here when it is not given)
        self.slot_order = slot_order
        self._row_maps = {}
        self._row_csrs = {}

    def row_map(self, Lc, n_cls):
        """int32 [N * (1 + Lc * P)]: for every token of the N = 2 * bs * rows / Lc sequences ``[CLS, Lc clips x P patches]`` its row in
        ``Xu = [n_cls CLS rows; bank[uniq]]`` viewed as [n_cls + n_unique * P, d].  Token (n, s > 0) -> n_cls + u * P + (s - 1) % P with
        u the place of its clip among the distinct ones; token (n, 0) -> row 0 when one CLS row serves every sequence (n_cls = 1,
        a learned token), else row n (n_cls = N: the mean of the sequence's own tokens)."""
        hit = self._row_maps.get((Lc, n_cls))
        if hit is None:
            P = int(self.bank.shape[1])
            N = self.inverse.numel() // Lc
            if n_cls not in (1, N):
                raise ValueError(f"row_map: {n_cls} CLS rows for {N} sequences (1 or {N})")
            tok = self.inverse.view(N, Lc, 1) * P + torch.arange(P, device=self.inverse.device) + n_cls
            cls = torch.arange(N, device=self.inverse.device).view(N, 1) if n_cls == N else tok.new_zeros((N, 1))
            hit = self._row_maps[(Lc, n_cls)] = torch.cat([cls, tok.view(N, Lc * P)], 1).reshape(-1).to(torch.int32)
        return hit

    def row_csr(self, Lc, n_cls):
        """``row_map(Lc, n_cls)`` turned round, as a CSR over the tokens: ``order`` int32 [N * S], the tokens sorted by their row of Xu
        with the tokens of one row in ascending order, and ``ptr`` int32 [n_cls + n_unique * P + 1], row r's tokens being
        ``order[ptr[r]:ptr[r + 1]]``.  The CLS rows come first (N groups of one token, or one group of N for a shared CLS row), then
        for distinct clip u and patch p the clip slots that hold u, in slot order - which is token order.  Index arithmetic on the
        device from the clip slots' stable argsort: no sort of the tokens, nothing read back."""
        hit = self._row_csrs.get((Lc, n_cls))
        if hit is None:
            P, nu, dev = int(self.bank.shape[1]), self.n_unique, self.inverse.device
            n = self.inverse.numel()
            N, S = n // Lc, 1 + Lc * P
            if n_cls not in (1, N):
                raise ValueError(f"row_csr: {n_cls} CLS rows for {N} sequences (1 or {N})")
            so = self.slot_order if self.slot_order is not None else torch.argsort(self.inverse, stable=True)
            inv_s = self.inverse[so]                                      # ascending: the slots of distinct clip 0, then of 1, ..
            cptr = torch.searchsorted(inv_s, torch.arange(nu + 1, device=dev))         # [nu + 1]: where clip u's slots start
            cnt = cptr[1:] - cptr[:-1]
            first, many = cptr[inv_s], cnt[inv_s]                         # per sorted slot: its clip's start and slot count
            p = torch.arange(P, device=dev)
            # sorted slot j, the t-th of clip u, patch p -> place N + first * P + p * many + t among the tokens, t = j - first
            pos = (N + first * (P - 1) + torch.arange(n, device=dev)).view(n, 1) + p * many.view(n, 1)
            tok = (torch.div(so, Lc, rounding_mode="floor") * S + 1 + (so % Lc) * P).view(n, 1) + p
            order = torch.empty(N * S, device=dev, dtype=torch.int64)
            order[:N] = torch.arange(N, device=dev) * S
            order.scatter_(0, pos.reshape(-1), tok.reshape(-1))
            cls = torch.arange(N, device=dev) if n_cls == N else torch.zeros(1, device=dev, dtype=torch.int64)
            clip = (N + cptr[:-1] * P).view(nu, 1) + p * cnt.view(nu, 1)
            ptr = torch.cat([cls, clip.reshape(-1), torch.full((1,), N * S, device=dev, dtype=torch.int64)])
            hit = self._row_csrs[(Lc, n_cls)] = (order.to(torch.int32), ptr.to(torch.int32))
        return hit

    def idx(self):
        n = self.bs * self.rows
        return self.idx_flat[self.kind * n:(self.kind + 1) * n]

    def materialize(self):
        from . import functional as F
        return F.gather_rows(self.bank, self.idx()).reshape(self.shape)

    def pairs_with(self, other) -> bool:
        """Is ``other`` the abnormal half of the batch this is the normal half of (one flat index vector, normal first)?"""
        return (isinstance(other, LazyRows) and other.idx_flat is self.idx_flat and self.kind == 0 and other.kind == 1 and
                (other.bs, other.rows) == (self.bs, self.rows))


def unique_clips(idx):
    """Sorted distinct entries of a clip-index array and, for every entry of ``idx.reshape(-1)``, its place among them (int64)."""
    uniq, inverse = np.unique(np.asarray(idx).reshape(-1), return_inverse=True)
    return uniq.astype(np.int64), inverse.reshape(-1).astype(np.int64)


class ResidentBank:
    """Features resident in HBM as ONE ``[total_clips, ...row]`` tensor; a training batch is formed on the device by
    ``lstc_gather_rows`` from clip indices the host sampler produced (MI355X-first data feed: a whole training set fits in
    288 GB, so no feature bytes cross PCIe per step).

    The index / label arrays of a step (a few tens of KB) travel through a ring of pinned host slabs with truly
    asynchronous copies on the compute stream, so the host keeps running ahead of the GPU (a pageable ``.to(device)`` would
    block the host until the previous step has drained)."""

    def __init__(self, bank: torch.Tensor, depth: int = 4):
        from . import functional as F
        self.F, self.bank, self.depth = F, bank, depth
        self._slot = 0
        self._pinned = [None] * depth
        self._done = [None] * depth

    def _stage(self, arrays):
        s = self._slot
        self._slot = (s + 1) % self.depth
        if self._done[s] is not None:
            self._done[s].synchronize()                 # the copies issued from this slab `depth` steps ago have completed
        slabs = self._pinned[s]
        if slabs is None or any(p.shape != tuple(a.shape) or p.numpy().dtype != a.dtype for p, a in zip(slabs, arrays)):
            slabs = self._pinned[s] = [torch.from_numpy(np.empty(a.shape, a.dtype)).pin_memory() for a in arrays]
        outs = []
        for p, a in zip(slabs, arrays):
            p.numpy()[...] = a
            outs.append(p.to(self.bank.device, non_blocking=True))
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.bank.device))
        self._done[s] = ev
        return outs

    def gather(self, idx, *extras, lazy=False):
        """``idx``: int64 numpy array of clip rows (any shape); returns ``bank[idx]`` with shape ``idx.shape + row`` plus the
        ``extras`` (small numpy arrays, e.g. labels) as device tensors.  ``lazy`` (``idx`` of shape [2, bs, rows]): the two
        halves come back as ``LazyRows`` - the indices are on the device, the rows are gathered by whoever consumes them."""
        # the fused gather reads bank[(idx * P + patch) ...] with no bound of its own (lstc_cls_concat_gather_fwd, lstc_gather_rows):
        # a stale or negative clip index would be a silent out-of-bounds read of HBM - reject it here, on a few hundred integers
        if idx.size and (int(idx.min()) < 0 or int(idx.max()) >= int(self.bank.shape[0])):
            raise IndexError(f"clip index out of range for a bank of {int(self.bank.shape[0])} clips: [{int(idx.min())}, {int(idx.max())}]")
        if lazy:
            if idx.ndim != 3 or idx.shape[0] != 2:
                raise ValueError("gather(lazy=True) takes the [2, bs, rows] index array of a normal / abnormal pair batch")
            # indices | distinct clips (padded to the same length: the slab keeps its shape from step to step) | inverse | the stable
            # argsort of inverse (the clip slots grouped by distinct clip, LazyRows.row_csr): ONE copy
            n = idx.size
            uniq, inverse = unique_clips(idx)
            staged = np.zeros(4 * n, np.int64)
            staged[:n], staged[n:n + uniq.size], staged[2 * n:3 * n] = idx.reshape(-1), uniq, inverse
            staged[3 * n:] = np.argsort(inverse, kind="stable")
            dev = self._stage([staged] + list(extras))
            flat, more = dev[0][:n], (dev[0][n:2 * n], dev[0][2 * n:3 * n], uniq.size, dev[0][3 * n:])
            pair = (LazyRows(self.bank, flat, 0, idx.shape[1], idx.shape[2], *more), LazyRows(self.bank, flat, 1, idx.shape[1], idx.shape[2], *more))
            pair[1]._row_maps, pair[1]._row_csrs = pair[0]._row_maps, pair[0]._row_csrs
            return (pair, *dev[1:])
        dev = self._stage([idx.reshape(-1)] + list(extras))
        out = self.F.gather_rows(self.bank, dev[0]).reshape(tuple(idx.shape) + tuple(self.bank.shape[1:]))
        return (out, *dev[1:])
