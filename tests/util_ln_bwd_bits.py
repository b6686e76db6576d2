"""The calls behind tests/golden/ln_bwd_bits.json: the three f32-row LayerNorm backward entry points of include/lstc_hip.h
(lstc_layernorm_bwd, lstc_layernorm_bwd_drop_pack, lstc_layernorm_bwd_drop) over the C ABI, with a SHA-256 digest of the raw bytes
of every output, and the return codes of the calls they refuse.

tools/record_ln_bwd_bits.py writes the digests of one build into the fixture; tests/test_ln_bwd_bits_gpu.py replays the calls and
compares.  Inputs come from numpy's seeded Mersenne Twister on the CPU; mean and rstd are float32 sums taken there in column
order (np.cumsum), so no forward kernel and no vectorised reduction has a part in a digest; output buffers start from a fixed
fill.  The calls:

  bwd        d = 4, 8, 100, 256, 260, 512, 516, 768, 1024, 1028, 2044, 2048: under each of the kernel's three vector widths the
             second wave of a row's pair owns no column, one float4 column, a part and all of its share; (rows, n_partial) =
             (1, 1), (5, 4) (more workgroups than row pairs: dead slots), (5, 1) (one workgroup walks every row), (37, 9).
  drop_pack  d = 64, 320, 512, 576, 1024, 1088, 2048 at rows = 256 (the pack's tile grid); n_partial = 1, 48 (uneven dealing, dead
             slots in the last trip), 200 (idle workgroups); p = 0 and 0.2.  The pack's digest covers its tile area.
  drop       d = 512, 1024, 2048; (rows, n_partial) = (5, 4), (37, 9); p = 0 and 0.2.

dx, df and the pack are recorded at every width.  The partial planes are recorded at d = 512 / 1024 / 2048 only: at the other
widths their summation order is not part of the contract (the column sums are held to float64 in tests/test_rowops_f64_gpu.py)."""
import hashlib
import itertools

import numpy as np
import torch

from lstc_vad_amd import _lib
from lstc_vad_amd._lib import check, stream_ptr

DEV = "cuda"
FILL = 7.0                      # what an output buffer holds before the call: a byte the kernel leaves alone stays in the digest
SEED = 20250311
EPS = 1e-6
DROP_SEED = 0x1234_5678_9ABC
MODEL_WIDTHS = (512, 1024, 2048)

BWD_D = (4, 8, 100, 256, 260, 512, 516, 768, 1024, 1028, 2044, 2048)
BWD_SHAPES = ((1, 1), (5, 4), (5, 1), (37, 9))
PACK_D = (64, 320, 512, 576, 1024, 1088, 2048)
PACK_ROWS, PACK_NP = 256, (1, 48, 200)
DROP_SHAPES = ((5, 4), (37, 9))
DROP_P = (0.0, 0.2)


def digest(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def ptr(t):
    return None if t is None else t.data_ptr()


def out(*shape):
    return torch.full(shape, FILL, dtype=torch.float32, device=DEV)


def inputs(name, rows, d):
    """dy, x, gamma, mean, rstd on the device; the statistics are float32 arithmetic in a fixed order on the CPU."""
    rng = np.random.RandomState(int.from_bytes(hashlib.sha256(f"{SEED}:{name}".encode()).digest()[:4], "little"))
    f32 = np.float32
    x = (f32(0.3) + f32(1.5) * rng.standard_normal((rows, d)).astype(f32)).astype(f32)
    dy = rng.standard_normal((rows, d)).astype(f32)
    gamma = (f32(1.0) + f32(0.5) * rng.standard_normal(d).astype(f32)).astype(f32)
    mean = (np.cumsum(x, axis=1, dtype=f32)[:, -1] / f32(d)).astype(f32)
    c = (x - mean[:, None]).astype(f32)
    var = (np.cumsum(c * c, axis=1, dtype=f32)[:, -1] / f32(d)).astype(f32)
    rstd = (f32(1.0) / np.sqrt(var + f32(EPS), dtype=f32)).astype(f32)
    return tuple(torch.from_numpy(a).to(DEV) for a in (dy, x, gamma, mean, rstd))


def _planes(key, d, partial):
    if d in MODEL_WIDTHS:
        yield key + "/partial", digest(partial)


def bwd_cases(lib):
    for d, (rows, n_partial) in itertools.product(BWD_D, BWD_SHAPES):
        key = f"bwd/d{d}/rows{rows}/np{n_partial}"
        dy, x, gamma, mean, rstd = inputs(key, rows, d)
        dx, partial = out(rows, d), out(2, n_partial, d)
        check(lib.lstc_layernorm_bwd(ptr(dy), ptr(x), ptr(gamma), ptr(mean), ptr(rstd), ptr(dx), ptr(partial), n_partial, rows, d,
                                     stream_ptr()), key)
        yield key + "/dx", digest(dx)
        yield from _planes(key, d, partial)


def drop_pack_cases(lib):
    rows = PACK_ROWS
    for d, n_partial, p in itertools.product(PACK_D, PACK_NP, DROP_P):
        key = f"drop_pack/d{d}/np{n_partial}/p{p}"
        dy, x, gamma, mean, rstd = inputs(key, rows, d)
        dx, partial = out(rows, d), out(3, n_partial, d)
        pk = torch.zeros(int(lib.lstc_pack1_bytes(rows, d)), device=DEV, dtype=torch.uint8)
        check(lib.lstc_layernorm_bwd_drop_pack(ptr(dy), ptr(x), ptr(gamma), ptr(mean), ptr(rstd), ptr(dx), ptr(partial), n_partial,
                                               rows, d, p, DROP_SEED, ptr(pk), stream_ptr()), key)
        yield key + "/dx", digest(dx)
        yield key + "/pack", digest(pk[:rows * d * 2])
        yield from _planes(key, d, partial)


def drop_cases(lib):
    for d, (rows, n_partial), p in itertools.product(MODEL_WIDTHS, DROP_SHAPES, DROP_P):
        key = f"drop/d{d}/rows{rows}/np{n_partial}/p{p}"
        dy, x, gamma, mean, rstd = inputs(key, rows, d)
        dx, df, partial = out(rows, d), out(rows, d), out(3, n_partial, d)
        check(lib.lstc_layernorm_bwd_drop(ptr(dy), ptr(x), ptr(gamma), ptr(mean), ptr(rstd), ptr(dx), ptr(df), ptr(partial),
                                          n_partial, rows, d, p, DROP_SEED, stream_ptr()), key)
        yield key + "/dx", digest(dx)
        yield key + "/df", digest(df)
        yield from _planes(key, d, partial)


def rc_cases(lib):
    """The return code of every kind of refusal, as a string.  All buffers have the size the named shape needs."""
    st = stream_ptr()

    def bufs(rows, d, n_partial=4):
        z = lambda *s: torch.zeros(*s, device=DEV)
        pk = torch.zeros(int(lib.lstc_pack1_bytes(rows, d)) + 16, device=DEV, dtype=torch.uint8)
        return [z(rows, d), z(rows, d), z(d), z(rows), z(rows)], z(rows * d + 4), z(rows, d), z(3, n_partial, d), pk

    def bwd(rows, d, n_partial=4, null=False, off=0):
        ins, dx, _, part, _ = bufs(rows, d, n_partial or 1)
        a = [ptr(t) for t in ins]
        return lib.lstc_layernorm_bwd(None if null else a[0], *a[1:], dx.data_ptr() + off, ptr(part), n_partial, rows, d, st)

    def drop_pack(rows, d, n_partial=4, p=0.2, null=False, off=0):
        ins, dx, _, part, pk = bufs(rows, d, n_partial or 1)
        return lib.lstc_layernorm_bwd_drop_pack(*(ptr(t) for t in ins), dx.data_ptr() + off, ptr(part), n_partial, rows, d, p,
                                                DROP_SEED, None if null else ptr(pk), st)

    def drop(rows, d, n_partial=4, p=0.2, null=False, off=0):
        ins, dx, df, part, _ = bufs(rows, d, n_partial or 1)
        return lib.lstc_layernorm_bwd_drop(*(ptr(t) for t in ins), dx.data_ptr() + off, None if null else ptr(df), ptr(part),
                                           n_partial, rows, d, p, DROP_SEED, st)

    cases = {
        "bwd/null": lambda: bwd(5, 512, null=True), "bwd/n_partial0": lambda: bwd(5, 512, 0),
        "bwd/d16388_lds_range": lambda: bwd(1, 16388), "bwd/d2052_generic": lambda: bwd(5, 2052),
        "bwd/unaligned_dx_generic": lambda: bwd(5, 512, off=4),
        "drop_pack/null": lambda: drop_pack(256, 512, null=True), "drop_pack/n_partial0": lambda: drop_pack(256, 512, 0),
        "drop_pack/p1": lambda: drop_pack(256, 512, p=1.0), "drop_pack/rows128": lambda: drop_pack(128, 512),
        "drop_pack/d516": lambda: drop_pack(256, 516), "drop_pack/d2112": lambda: drop_pack(256, 2112),
        "drop_pack/unaligned_dx": lambda: drop_pack(256, 512, off=4),
        "drop/null": lambda: drop(5, 512, null=True), "drop/n_partial0": lambda: drop(5, 512, 0), "drop/p1": lambda: drop(5, 512, p=1.0),
        "drop/d768": lambda: drop(5, 768), "drop/d516": lambda: drop(5, 516), "drop/unaligned_dx": lambda: drop(5, 512, off=4),
    }
    for name, call in cases.items():
        rc = call()
        torch.cuda.synchronize()
        yield "rc/" + name, str(int(rc))


def all_digests():
    """{call id / output: sha256 hex, or the return code of a refused call} on the loaded library."""
    lib = _lib.load()
    res = {}
    for k, v in itertools.chain(bwd_cases(lib), drop_pack_cases(lib), drop_cases(lib), rc_cases(lib)):
        assert k not in res, k
        res[k] = v
    return res
