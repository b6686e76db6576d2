"""The calls behind tests/golden/cls_concat_bits.json: every CLS-concat entry point of include/lstc_hip.h (fixed, pack, gather, len,
var; forward and backward) and the three f32 CLS passes (lstc_cls_dot / _len / _var, lstc_cls_wsum / _var, lstc_cls_outer / _var)
over the C ABI, at the smallest shapes that reach each path, with a SHA-256 digest of the raw bytes of every output.

tools/record_cls_concat_bits.py writes the digests of one build into the fixture; tests/test_cls_layouts_gpu.py replays the calls
and compares.  Inputs come from numpy's seeded Mersenne Twister on the CPU, output buffers start from a fixed fill, so a digest
depends on the kernels alone.  The shapes:

  concat   N = 3; d = 36 (16-B path, one partial workgroup), 30 (4-B path), 1028 (dv = 257: a second column group with one live
           lane), and d = 36 with every float operand 4 bytes off a 16-B boundary; S - 1 = 1, 8, 17 (one token, exactly one trip of
           the unrolled token loop, two trips and a remainder); lengths [1, 9, S - 1] (len: 9 > S - 1 meets the clamp; var: the
           real min(9, S - 1)), NaN in the padding of x; learned / mean CLS, with and without pos; n_lo = 0, 1, N; pack and pack-only
           at N = 16, S = 16, d = 64 (the smallest that fills the 256-row, 64-column pack grid); gather at P = 2 with two clips per
           sequence and a repeated clip index.
  passes   (N, S, H, d) = (3, 2, 2, 64) and (3, 65, 8, 64) (one key beyond a 64-lane wave), lengths [1, 2, S]; lstc_cls_dot in
           modes 0, 1, 2 with dropout 0 and 0.25."""
import hashlib
import itertools

import numpy as np
import torch

from lstc_vad_amd import _lib
from lstc_vad_amd._lib import check, stream_ptr

DEV = "cuda"
FILL = 7.0                      # what an output buffer holds before the call: a byte the kernel leaves alone stays in the digest
SEED = 20240607


def digest(*tensors):
    h = hashlib.sha256()
    torch.cuda.synchronize()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


class Gen:
    """Seeded CPU generator; ``off`` puts every float tensor 4 bytes off a 16-B boundary."""

    def __init__(self, name, off=False):
        self.rng = np.random.RandomState(int.from_bytes(hashlib.sha256(f"{SEED}:{name}".encode()).digest()[:4], "little"))
        self.off = off

    def _place(self, host):
        if not self.off:
            return host.to(DEV)
        buf = torch.empty(host.numel() + 4, device=DEV, dtype=host.dtype)
        assert buf.data_ptr() % 16 == 0
        out = buf[1:1 + host.numel()].view(host.shape)
        out.copy_(host)
        return out

    def randn(self, *shape):
        return self._place(torch.from_numpy(self.rng.standard_normal(shape).astype(np.float32)))

    def out(self, *shape):
        return self._place(torch.full(shape, FILL, dtype=torch.float32))


def ptr(t):
    return None if t is None else t.data_ptr()


def i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _row0(lens):
    return [0] + list(itertools.accumulate(L + 1 for L in lens))


# ------------------------------------------------------------------------------------------------------------ CLS concat
CONCAT_D = (("d36", 36, False), ("d30", 30, False), ("d1028", 1028, False), ("d36off", 36, True))
CONCAT_L = (1, 8, 17)
N3 = 3


def _concat_plain(lib, name, d, off, L, learned, with_pos):
    """(key, digest) of the fixed, len and var calls of one (d, L, cls, pos) cell."""
    g = Gen(name, off)
    S = L + 1
    x = g.randn(N3, L, d)
    cls = g.randn(d) if learned else None
    pos = g.randn(S, d) if with_pos else None
    dy = g.randn(N3, S, d)
    mean_cls = 0 if learned else 1
    st = stream_ptr()

    y = g.out(N3, S, d)
    check(lib.lstc_cls_concat_fwd(ptr(x), None, 0, ptr(cls), ptr(pos), ptr(y), N3, S, d, st), "cls_concat_fwd")
    yield f"fwd/{name}", digest(y)
    if L == 8:      # the split batch: sequences [0, n_lo) from x, the rest from x_hi
        for n_lo in (0, 1, N3):
            y = g.out(N3, S, d)
            hi = x.data_ptr() + n_lo * L * d * 4
            check(lib.lstc_cls_concat_fwd(ptr(x), hi, n_lo, ptr(cls), ptr(pos), ptr(y), N3, S, d, st), "cls_concat_fwd")
            yield f"fwd/{name}/n_lo{n_lo}", digest(y)
    dx = g.out(N3, L, d)
    check(lib.lstc_cls_concat_bwd(ptr(dy), ptr(dx), N3, S, d, mean_cls, st), "cls_concat_bwd")
    yield f"bwd/{name}", digest(dx)

    # padded: lengths [1, 9, L] as given (the kernel clamps to [1, L]), NaN behind a sequence's own tokens
    lens = [1, 9, L]
    real = [min(max(v, 1), L) for v in lens]
    xp = x.clone() if not off else g._place(x.cpu())
    for n, v in enumerate(real):
        xp[n, v:] = float("nan")
    lt = i32(lens)
    y = g.out(N3, S, d)
    check(lib.lstc_cls_concat_len_fwd(ptr(xp), ptr(lt), ptr(cls), ptr(pos), ptr(y), N3, S, d, st), "cls_concat_len_fwd")
    yield f"len_fwd/{name}", digest(y)
    dx, dtok = g.out(N3, L, d), g.out(S, d)
    check(lib.lstc_cls_concat_len_bwd(ptr(dy), ptr(lt), ptr(dx), ptr(dtok), N3, S, d, mean_cls, st), "cls_concat_len_bwd")
    yield f"len_bwd/{name}", digest(dx, dtok)

    # unpadded: the same sequences back to back
    r0 = _row0(real)
    rt = i32(r0)
    xv = g._place(torch.cat([x[n, :v].cpu() for n, v in enumerate(real)], 0))
    dyv = g._place(torch.cat([dy[n, :v + 1].cpu() for n, v in enumerate(real)], 0))
    y = g.out(r0[-1], d)
    check(lib.lstc_cls_concat_var_fwd(ptr(xv), ptr(rt), ptr(cls), ptr(pos), ptr(y), N3, d, st), "cls_concat_var_fwd")
    yield f"var_fwd/{name}", digest(y)
    S_max = max(real) + 1
    dx, dtok = g.out(r0[-1] - N3, d), g.out(S_max, d)
    check(lib.lstc_cls_concat_var_bwd(ptr(dyv), ptr(rt), ptr(dx), ptr(dtok), N3, S_max, d, mean_cls, st), "cls_concat_var_bwd")
    yield f"var_bwd/{name}", digest(dx, dtok)
    if L == 8:      # one output alone: the other's launch is skipped and its null pointer counts as aligned
        dx, dtok = g.out(N3, L, d), g.out(S, d)
        check(lib.lstc_cls_concat_len_bwd(ptr(dy), ptr(lt), ptr(dx), None, N3, S, d, mean_cls, st), "cls_concat_len_bwd")
        check(lib.lstc_cls_concat_len_bwd(ptr(dy), ptr(lt), None, ptr(dtok), N3, S, d, mean_cls, st), "cls_concat_len_bwd")
        yield f"len_bwd/{name}/single", digest(dx, dtok)
        dx, dtok = g.out(r0[-1] - N3, d), g.out(S_max, d)
        check(lib.lstc_cls_concat_var_bwd(ptr(dyv), ptr(rt), ptr(dx), None, N3, S_max, d, mean_cls, st), "cls_concat_var_bwd")
        check(lib.lstc_cls_concat_var_bwd(ptr(dyv), ptr(rt), None, ptr(dtok), N3, S_max, d, mean_cls, st), "cls_concat_var_bwd")
        yield f"var_bwd/{name}/single", digest(dx, dtok)


def _concat_pack(lib, name, off, learned, with_pos):
    """lstc_cls_concat_fwd_pack and the gather entry with a pack at N = 16, S = 16, d = 64."""
    N, S, d, P = 16, 16, 64, 5
    g = Gen(name, off)
    x = g.randn(N, S - 1, d)
    cls = g.randn(d) if learned else None
    pos = g.randn(S, d) if with_pos else None
    nbytes = int(lib.lstc_pack1_bytes(N * S, d))
    st = stream_ptr()
    pack = lambda: torch.zeros(nbytes, device=DEV, dtype=torch.uint8)
    for n_lo in (None, 8):
        hi = None if n_lo is None else x.data_ptr() + n_lo * (S - 1) * d * 4
        y, pk = g.out(N, S, d), pack()
        check(lib.lstc_cls_concat_fwd_pack(ptr(x), hi, n_lo or 0, ptr(cls), ptr(pos), ptr(y), N, S, d, ptr(pk), st), "fwd_pack")
        yield f"fwd_pack/{name}/n_lo{n_lo}", digest(y, pk)
        if not off:     # pack only exists on the 16-B path
            pk = pack()
            check(lib.lstc_cls_concat_fwd_pack(ptr(x), hi, n_lo or 0, ptr(cls), ptr(pos), None, N, S, d, ptr(pk), st), "fwd_pack")
            yield f"fwd_pack_only/{name}/n_lo{n_lo}", digest(pk)
    if not off:
        clips = 7
        bank = g.randn(clips, P, d)
        idx = torch.from_numpy(g.rng.randint(0, clips, size=N * (S - 1) // P).astype(np.int64)).to(DEV)
        y, pk = g.out(N, S, d), pack()
        check(lib.lstc_cls_concat_gather_fwd(ptr(bank), clips, ptr(idx), P, ptr(cls), ptr(pos), ptr(y), N, S, d, ptr(pk), st), "gather")
        yield f"gather_pack/{name}", digest(y, pk)
        pk = pack()
        check(lib.lstc_cls_concat_gather_fwd(ptr(bank), clips, ptr(idx), P, ptr(cls), ptr(pos), None, N, S, d, ptr(pk), st), "gather")
        yield f"gather_pack_only/{name}", digest(pk)


def _concat_gather(lib, name, d, learned, with_pos):
    """P = 2, two clips per sequence (S - 1 = 4), clip 3 read by two sequences and clip 0 twice by one."""
    N, S, P, clips = 3, 5, 2, 4
    g = Gen(name)
    bank = g.randn(clips, P, d)
    cls = g.randn(d) if learned else None
    pos = g.randn(S, d) if with_pos else None
    idx = torch.tensor([0, 0, 3, 1, 2, 3], dtype=torch.int64, device=DEV)
    y = g.out(N, S, d)
    check(lib.lstc_cls_concat_gather_fwd(ptr(bank), clips, ptr(idx), P, ptr(cls), ptr(pos), ptr(y), N, S, d, None, stream_ptr()), "gather")
    yield f"gather/{name}", digest(y)


def concat_cases(lib):
    for (dname, d, off), L, learned, with_pos in itertools.product(CONCAT_D, CONCAT_L, (False, True), (False, True)):
        yield from _concat_plain(lib, f"{dname}/L{L}/{'learned' if learned else 'mean'}/{'pos' if with_pos else 'nopos'}", d, off, L,
                                 learned, with_pos)
    for off, learned, with_pos in itertools.product((False, True), (False, True), (False, True)):
        yield from _concat_pack(lib, f"{'off' if off else 'aligned'}/{'learned' if learned else 'mean'}/{'pos' if with_pos else 'nopos'}",
                                off, learned, with_pos)
    for d, learned, with_pos in itertools.product((36, 1028), (False, True), (False, True)):
        yield from _concat_gather(lib, f"d{d}/{'learned' if learned else 'mean'}/{'pos' if with_pos else 'nopos'}", d, learned, with_pos)


# ------------------------------------------------------------------------------------------------------------ CLS passes
PASS_SHAPES = ((3, 2, 2, 64), (3, 65, 8, 64))
DROP_SEED = 0x1234_5678_9ABC


def _passes(lib, N, S, H, d):
    name = f"N{N}S{S}H{H}d{d}"
    g = Gen("passes/" + name)
    st = stream_ptr()
    klen = [1, 2, S]
    r0 = [0] + list(itertools.accumulate(klen))
    U, X = g.randn(N, H, d), g.randn(N, S, d)
    W1, W2, U2, add0 = g.randn(N, H, S), g.randn(N, H, S), g.randn(N, H, d), g.randn(N, d)
    Xl = X.clone()
    for n, v in enumerate(klen):
        Xl[n, v:] = float("nan")
    Xv = torch.cat([X[n, :v] for n, v in enumerate(klen)], 0).contiguous()
    kt, rt = i32(klen), i32(r0)

    def dot(layout, mode, probs, p):
        out = g.out(N, H, S)
        a = (N, S, H, d, mode, p, DROP_SEED, st)
        if layout == "fixed":
            check(lib.lstc_cls_dot(ptr(U), ptr(X), ptr(out), ptr(probs), *a), "cls_dot")
        elif layout == "len":
            check(lib.lstc_cls_dot_len(ptr(U), ptr(Xl), ptr(kt), ptr(out), ptr(probs), *a), "cls_dot_len")
        else:
            check(lib.lstc_cls_dot_var(ptr(U), ptr(Xv), ptr(rt), ptr(out), ptr(probs), *a), "cls_dot_var")
        return out

    for layout in ("fixed", "len", "var"):
        yield f"dot_{layout}/{name}/mode0", digest(dot(layout, 0, None, 0.0))
        for p in (0.0, 0.25):
            probs = g.out(N, H, S)
            out = dot(layout, 1, probs, p)
            yield f"dot_{layout}/{name}/mode1/p{p}", digest(out, probs)
            yield f"dot_{layout}/{name}/mode2/p{p}", digest(dot(layout, 2, probs, p))

    # wsum / outer: the weights of the len form are zero behind a sequence's keys, which is how the fixed entry serves it
    Y = g.out(N, H, d)
    check(lib.lstc_cls_wsum(ptr(W1), ptr(X), ptr(Y), N, S, H, d, st), "cls_wsum")
    yield f"wsum_fixed/{name}", digest(Y)
    Y = g.out(N, H, d)
    check(lib.lstc_cls_wsum_var(ptr(W1), ptr(Xv), ptr(rt), ptr(Y), N, S, H, d, st), "cls_wsum_var")
    yield f"wsum_var/{name}", digest(Y)
    dX = g.out(N, S, d)
    check(lib.lstc_cls_outer(ptr(W1), ptr(U), ptr(W2), ptr(U2), ptr(dX), N, S, H, d, st), "cls_outer")
    yield f"outer_fixed/{name}", digest(dX)
    for a0 in (None, add0):
        dX = g.out(r0[-1], d)
        check(lib.lstc_cls_outer_var(ptr(W1), ptr(U), ptr(W2), ptr(U2), ptr(a0), ptr(rt), ptr(dX), N, S, H, d, st), "cls_outer_var")
        yield f"outer_var/{name}/{'add0' if a0 is not None else 'noadd'}", digest(dX)


def pass_cases(lib):
    for shape in PASS_SHAPES:
        yield from _passes(lib, *shape)


def all_digests():
    """{call id: sha256 hex} of every call above on the loaded library."""
    lib = _lib.load()
    out = {}
    for k, v in itertools.chain(concat_cases(lib), pass_cases(lib)):
        assert k not in out, k
        out[k] = v
    return out
