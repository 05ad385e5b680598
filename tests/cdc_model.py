"""Reference model of content-defined chunking (include/cw_hashcompress.h).

``chunk`` is the numpy restatement: the window hash H of every position, vectorised over the 64 shifted gear terms, then
the cut chain over the sorted candidate positions.  ``chunk_serial`` is the plain loop written straight from the
definition, for cross-checking ``chunk`` on small inputs."""
from __future__ import annotations

import numpy as np

M64 = (1 << 64) - 1


def splitmix64(x: int) -> int:
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


GEAR = np.array([splitmix64(v) for v in range(256)], dtype=np.uint64)


def top_bits(k: int) -> int:
    return (M64 << (64 - k)) & M64 if k > 0 else 0


def default_params(normal: int) -> dict:
    lg = normal.bit_length() - 1
    return dict(min=normal // 4, avg=normal, max=normal * 8, mask_s=top_bits(lg + 2), mask_l=top_bits(lg - 2), gear=None)


def params(min_size, avg, max_size, mask_s, mask_l, gear=None) -> dict:
    return dict(min=min_size, avg=avg, max=max_size, mask_s=mask_s, mask_l=mask_l, gear=gear)


def _gear(p):
    return GEAR if p.get("gear") is None else np.asarray(p["gear"], dtype=np.uint64)


def window_hash(b: np.ndarray, gear=GEAR) -> np.ndarray:
    g = gear[b]
    h = np.zeros(len(b), dtype=np.uint64)
    with np.errstate(over="ignore"):
        for k in range(min(64, len(b))):
            h[k:] += g[: len(b) - k] << np.uint64(k)
    return h


def chunk(data, p: dict, final: bool = True) -> list[int]:
    """Cuts c_0 = 0 .. c_K.  final = False: the chain stops at the first cut c with c + max > n (c = bytes consumed)."""
    a = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data.reshape(-1).view(np.uint8)
    n = len(a)
    H = window_hash(a, _gear(p))
    cs = np.flatnonzero((H & np.uint64(p["mask_s"])) == 0) + 1  # cut x is a candidate when H(x-1) & mask == 0
    cl = np.flatnonzero((H & np.uint64(p["mask_l"])) == 0) + 1
    m, A, M = p["min"], p["avg"], p["max"]
    cuts, c = [0], 0
    while True:
        if (c == n) if final else (c + M > n):
            return cuts
        r = n - c
        if r <= m:
            c = n
        else:
            e, z = c + min(M, r), c + min(A, r)
            i = np.searchsorted(cs, c + m)
            if i < len(cs) and cs[i] < z:
                c = int(cs[i])
            else:
                j = np.searchsorted(cl, z)
                c = int(cl[j]) if j < len(cl) and cl[j] < e else e
        cuts.append(c)


def chunk_serial(data: bytes, p: dict, final: bool = True) -> list[int]:
    """The definition as a plain loop."""
    gear = [int(v) for v in _gear(p)]
    n = len(data)
    H, h = [0] * n, 0
    for i in range(n):
        h = ((h << 1) + gear[data[i]]) & M64
        H[i] = h
    cuts, c = [0], 0
    while not ((c == n) if final else (c + p["max"] > n)):
        r = n - c
        if r <= p["min"]:
            c = n
        else:
            e, z = c + min(p["max"], r), c + min(p["avg"], r)
            x = e
            for y in range(c + p["min"], e):
                if H[y - 1] & (p["mask_s"] if y < z else p["mask_l"]) == 0:
                    x = y
                    break
            c = x
        cuts.append(c)
    return cuts


def chunk_pieces(data: bytes, p: dict, sizes) -> list[int]:
    """The streaming contract: pieces of the given sizes, final = False until the last; the bytes after each piece's last
    cut are carried into the next call."""
    cuts, done, pos = [0], 0, 0
    sizes = list(sizes)
    while True:
        pos = min(len(data), pos + (sizes.pop(0) if sizes else len(data)))
        fin = pos == len(data)
        part = chunk(data[done:pos], p, final=fin)
        cuts += [done + x for x in part[1:]]
        done += part[-1]
        if fin:
            return cuts
