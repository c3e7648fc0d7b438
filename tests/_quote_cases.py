"""Contents shared by the quote kernel's CPU model tests (test_quote_model.py) and GPU tests (test_gpu_quote.py)."""
import numpy as np

# as in test_gpu_quote.py
ALPHABET = np.frombuffer(b'"\n,a', np.uint8)
SPARSE = np.frombuffer(b'"\n,,' + b"a" * 28, np.uint8)


def one_lane_16(n: int, seed: int) -> np.ndarray:
    """Text in which, per 1 KiB wave row, exactly one 16-byte chunk is sixteen newlines and no other byte is one
    (phase B's 5-bit ballot path with a single lane holding the maximum); a few quotes between them, so that both
    incoming states occur."""
    rng = np.random.default_rng(seed)
    d = np.full(n, 97, np.uint8)
    d[rng.integers(0, max(n, 1), n // 3000)] = 34
    for r in range(n // 1024 + 1):
        c = r * 1024 + 16 * int(rng.integers(0, 64))
        d[c:c + 16] = 10                                 # clipped by the end of the array
    return d


def mixed_0_1_16(n: int, seed: int) -> np.ndarray:
    """Every 16-byte chunk holds no newline, exactly one, or sixteen (rows that mix the counts 0, 1 and 16; every
    fourth 1 KiB row only 0 and 1, the one-ballot path), and one chunk in 50 a quote."""
    rng = np.random.default_rng(seed)
    m = n // 16 + 1
    d = np.full((m, 16), 97, np.uint8)
    kind = rng.choice(3, m, p=[0.6, 0.3, 0.1])
    kind[(kind == 2) & ((np.arange(m) // 64) % 4 == 3)] = 1
    one = np.flatnonzero(kind == 1)
    d[one, rng.integers(0, 16, len(one))] = 10
    d[kind == 2] = 10
    q = np.flatnonzero((kind == 0) & (rng.random(m) < 0.02))
    d[q, rng.integers(0, 16, len(q))] = 34
    return d.reshape(-1)[:n].copy()


def odd_tiles(n: int, tile: int, seed: int) -> np.ndarray:
    """SPARSE text of ``n`` bytes in which every ``tile``-byte block has an odd number of quotes."""
    rng = np.random.default_rng(seed)
    d = SPARSE[rng.integers(0, 32, n, dtype=np.uint8)].copy()
    for t0 in range(0, n, tile):
        blk = d[t0:t0 + tile]
        if np.count_nonzero(blk == 34) % 2 == 0:
            blk[int(np.flatnonzero(blk == 97)[0])] = 34
    return d


def every_value_every_position(n: int = 4096) -> np.ndarray:
    """``n`` = 4096 bytes in which each of the 256 byte values occurs at each position mod 16: value
    (37 * i + i // 256) mod 256 at index i -- a stride coprime to 256 visits every value once per 256 bytes, and the
    shift by one per 256 bytes moves each value through the 16 positions."""
    i = np.arange(n)
    return ((37 * i + i // 256) & 0xFF).astype(np.uint8)
