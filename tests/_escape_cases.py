"""Inputs of the escape-aware record index tests, shared by the lane-model tests (CPU) and the kernel tests (GPU).

A case is a dict: buf (uint8, object bytes [base, base + len)), base, begin, end, quote, escape, carry, esc_carry,
scope, forms (the output forms it can run in).  The device address of buf[0] is congruent to ``base`` mod 16 in every
test, so ``begin & 15`` is the alignment of the first byte in its chunk and the blocked form's rule holds.
"""
import numpy as np

T = 1 << 16
Q, E, NL = 34, 92, 10
PLAIN = np.frombuffer(b'"\n,a', np.uint8)                # no escape byte
FIVE = np.frombuffer(b'"\\\n,a', np.uint8)               # the five-symbol alphabet {q, e, '\n', ',', 'a'}
ALL_FORMS = ("u32", "u64", "u16b")

EDGES_ODD = (T + 15, T + 1023, T + 16383, 2 * T - 1)     # offsets 15, 1023, 16383, 65535 of a tile
EDGES_EVEN = (T + 16, T + 1024, T + 16384, 2 * T)        # offsets 16, 1024, 16384, 65536
RUN_LENGTHS = tuple(range(1, 35))
EXACT_RUNS = (16, 32, 1024, 16384, 65536)


def case(buf, begin=0, end=None, carry=0, esc_carry=0, scope="all", escape=E, quote=Q, base=0, forms=ALL_FORMS,
         name=""):
    buf = np.ascontiguousarray(buf, np.uint8)
    return dict(buf=buf, base=base, begin=begin, end=base + len(buf) if end is None else end, quote=quote,
                escape=escape, carry=carry, esc_carry=esc_carry, scope=scope, forms=forms, name=name)


def plain(n, seed):
    return PLAIN[np.random.default_rng(seed).integers(0, 4, n)]


def after_run(d, p):
    """A quote, a newline and another quote right behind a run that ends before p: whether the quote at p is
    escaped decides every later record end."""
    d[p:p + 3] = (Q, NL, Q)


def edge_cases(edges):
    """Escape runs of every length 1..34 that end just before each of ``edges`` (one buffer per length)."""
    out = []
    for L in RUN_LENGTHS:
        d = plain(2 * T + 64, L)
        for e in edges:
            d[e - L:e] = E
            d[e - L - 1] = ord("a")                      # the run is maximal: exactly L bytes
            after_run(d, e)
        out.append(case(d, scope="all" if L % 2 else "quoted", name=f"run{L}"))
    return out


def exact_run_cases():
    """Runs of exactly 16, 32, 1024, 16 KiB and 64 KiB bytes and each plus one, chunk-aligned and not."""
    out = []
    for L in EXACT_RUNS:
        for extra in (0, 1):
            for start in (T, T + 7):
                d = plain(start + L + extra + T // 2 + 9, L + extra + start)
                d[start - 1] = ord("a")
                d[start:start + L + extra] = E
                after_run(d, start + L + extra)
                out.append(case(d, name=f"exact{L}+{extra}@{start - T}"))
    return out


def all_escape_tile_cases():
    """A whole tile of escape bytes between two ordinary ones, entered with the flag clear and set."""
    out = []
    for odd in (0, 1):
        d = plain(3 * T, 77 + odd)
        d[T:2 * T] = E
        d[T - 2] = ord("a")
        d[T - 1] = E if odd else ord("a")                # odd: the tile's first byte is escaped, and so is the quote
        after_run(d, 2 * T)                              # behind the run of 65537
        out.append(case(d, name=f"all_escape_tile_in{odd}"))
    return out


def alignment_cases():
    """begin at each of the 16 alignments, both carries, both esc_carries, both scopes; the bytes at begin are
    escape bytes, quotes and newlines, so esc_carry decides."""
    out = []
    rng = np.random.default_rng(5)
    for al in range(16):
        for carry in (0, 1):
            for ec in (0, 1):
                for scope in ("all", "quoted"):
                    n = 1100 + al * 3
                    d = FIVE[rng.choice(5, n, p=(0.2, 0.35, 0.2, 0.1, 0.15))]
                    lead = (Q, NL, E)[(al + carry) % 3]
                    d[al] = lead
                    if al % 4 == 1:
                        d[al:16] = E                     # the rest of the first chunk: escape bytes from begin on
                    out.append(case(d, begin=al, end=n - (al % 5), carry=carry, esc_carry=ec, scope=scope,
                                    name=f"al{al}c{carry}e{ec}{scope}"))
    return out


def blocked_large_begin_cases():
    """The u16b form entered far into its first 64 KiB block, at object offsets above 2^32."""
    out = []
    rng = np.random.default_rng(9)
    for k, b0 in enumerate((65520, 65535, 65521 - 16384, 40000)):
        n = T + 300 + k
        d = FIVE[rng.choice(5, n + 40, p=(0.2, 0.3, 0.2, 0.1, 0.2))]
        base = 70_001 * T + b0 - 20                      # base and begin congruent to each other's low bits mod 16
        if k % 2:
            d[20:20 + 16 - (b0 & 15)] = E                # escape bytes from begin to the end of its chunk
        out.append(case(d, begin=base + 20, end=base + 20 + n, base=base, carry=k & 1, esc_carry=1,
                        scope="quoted" if k & 2 else "all", forms=("u64", "u16b"), name=f"blocked_b0_{b0}"))
    return out


def random_five(n, seed, p=(0.2, 0.25, 0.2, 0.15, 0.2)):
    return FIVE[np.random.default_rng(seed).choice(5, n, p=p)]


# ------------------------------------------------------------------------------------------ oracle and model of a case
def expect(c):
    """(record ends uint64, n_quotes, n_newlines, toggles) of a case by the byte loop (tests/_escape_loop.py)."""
    from _escape_loop import loop_newlines, loop_quote_bytes, loop_record_ends
    ends, toggles, _, _ = loop_record_ends(c["buf"], c["begin"], c["end"], c["quote"], c["escape"], c["carry"],
                                           c["esc_carry"], c["scope"], c["base"])
    return ends, loop_quote_bytes(c["buf"], c["begin"], c["end"], c["quote"], c["base"]), \
        loop_newlines(c["buf"], c["begin"], c["end"], c["quote"], c["escape"], c["esc_carry"], c["scope"],
                      c["base"]), toggles


def model(emu, c, form="u64", schedule="sequential", mutate=None):
    """The lane model's launch of a case in one output form: (out..., n_out, n_quotes, n_newlines, err, toggles)."""
    st = {}
    r = emu.run(c["buf"], dev_addr=c["base"] % 16, buf_base=c["base"], begin=c["begin"], end=c["end"],
                quote=c["quote"], carry=c["carry"], u64=form != "u32", schedule=schedule, mutate=mutate, stats=st,
                fmt="u16b" if form == "u16b" else None, escape=c["escape"], esc_carry=c["esc_carry"],
                escape_scope=c["scope"])
    return r + (st["n_toggles"],)


def check_model(emu, c, exp=None, forms=None, schedule="sequential"):
    """The model of a case equals the loop in every form the case runs in."""
    from _escape_loop import blocked
    ends, nq, nn, tog = exp or expect(c)
    for form in forms or c["forms"]:
        r = model(emu, c, form, schedule)
        assert r[-5:] == (len(ends), nq, nn, 0, tog), (c["name"], form, r[-5:], (len(ends), nq, nn, 0, tog))
        if form == "u16b":
            low, table = blocked(ends, c["begin"], c["end"])
            assert np.array_equal(r[0], low) and np.array_equal(r[1], table), (c["name"], form)
        else:
            assert r[0].dtype == (np.uint64 if form == "u64" else np.uint32)
            assert np.array_equal(r[0].astype(np.uint64), ends), (c["name"], form)
