"""Built inputs that put the scan kernels (dataplug_amd/csrc/dpscan.hip) on every threshold their code branches on.

Shared by the CPU test (test_scan_cases_cpu.py: the drift guard, every case's property checked numerically from the
oracle's index) and the GPU test (test_gpu_scan_edges.py).  No GPU imports.

Coordinates.  The kernels work in *aligned coordinates*: offsets from the device address of the buffer rounded down
to 16 bytes, so buffer byte i sits at aligned i + shift (shift = device address mod 16) and range r of a chunk that
starts at buffer byte 0 covers aligned [r * RANGE, (r + 1) * RANGE).  Every builder takes ``shift`` and places its
structure by aligned coordinate; ``data[x - shift]`` is the byte at aligned x.  FASTA cases are uploaded at
``shift`` with buf_base 0 (object offset = aligned - shift); newline cases with buf_base = shift, so that their
object offsets ARE the aligned coordinates (out_mode 3 / 4 need the two congruent mod 16, and their 64 KiB / 256-byte
tables are in object offsets).

A case is ``Case(name, kind, build, plans, prop, shift, extra)``: ``data`` builds the bytes on demand (the 17 MiB
cases are not kept alive), ``plans`` is a list of chunk plans (FASTA), of ``(lo, hi)`` range lists in object offsets
(newline) or of ``from`` offsets (find); ``prop`` is the machine-checkable claim the case exists for.
"""
from collections import namedtuple

import numpy as np

from _quote_cases import every_value_every_position

# ---------------------------------------------------------------------------------------------- geometry (dpscan.hip)
LANE = 16                     # bytes per lane and load (kRowBytes / kWave)
ROW = 1024                    # kRowBytes: one wave-wide load
BUF = 8 << 10                 # kBufBytes: rows in flight per buffer
RANGE = 16384                 # kWaveBytes: one wave's range, one summary record
GROUP_RANGES = 16             # kMapWaves: ranges per map_kernel / line_kernel group
UNIT_RANGES = 15              # kDataWaves: ranges per one-pass look-back unit
PLACE_BLOCK = 1024            # kPlaceBlock: range records per placement block
STAGE_BYTES = 128 << 10       # kStageBytes: LDS staging of a placement block's output run
SPILL_CAP = 512               # kSpillCap: events kept per range by map_kernel; more = dense
PREFETCH_EVENTS = 32          # events of the four spill words (sw0..sw3) loaded with a range's record
LINE_CAP = 640                # kLineCap: positions kept per range by line_kernel; more = dense
DENSE_MAX = 1024              # kDenseMax: events kept per range by the one-pass kernel; more = dense
GROUP = GROUP_RANGES * RANGE  # 256 KiB
UNIT = UNIT_RANGES * RANGE    # 240 KiB
BLOCK = PLACE_BLOCK * RANGE   # 16 MiB

GT, NL, A_, H_, X_ = 62, 10, 65, 104, 120
DELIM_BYTES = (0x00, 0x0A, 0x0C, 0x80, 0xFF)      # 0x0C: the v_perm zero selector (key = pattern ^ 0x0C0C0C0C)

F_COUNT_EVENTS = (30, 31, 32, 33, 34, 510, 511, 512, 513, 514, 1022, 1023, 1024, 1025, 1026)
F_COUNT_RANGES = (0, GROUP_RANGES - 1, GROUP_RANGES)   # range 0; last of group 0 = first of one-pass unit 1; first of group 1
F_RUN_PAIRS = (16383, 16384, 16385, 8191, 8192, 8193)  # kStageBytes in uint32 pairs +- 1, in uint64 pairs +- 1
D_COUNT_DELIMS = (0, 1, 639, 640, 641, 1023, 1024, 1025, 16384)
D_COUNT_RANGES = (0, GROUP_RANGES - 1, GROUP_RANGES)
BOUNDARIES = ("lane", "row", "buffer", "range", "unit", "group", "block", "chunk", "object")
FIND_SHIFTS = (0, 5, 15)
FIND_SCENARIOS = ("at_from", "before_from", "last_byte", "past_buf_len", "second_step", "third_step")


class Case(namedtuple("Case", "name kind build plans prop shift extra")):
    __slots__ = ()

    @property
    def data(self) -> np.ndarray:
        return self.build()


def _case(name, kind, build, plans, prop, shift=0, **extra):
    return Case(name, kind, build, plans, prop, shift, extra)


# ---------------------------------------------------------------------------------------------- backgrounds
def fasta_bg(n: int) -> np.ndarray:
    """``ACGT`` with a newline every 61 bytes: no '>' anywhere, so only built structure makes events."""
    a = np.tile(np.frombuffer(b"ACGT", np.uint8), n // 4 + 1)[:n].copy()
    a[60::61] = NL
    return a


class _Obj:
    """Bytes addressed by aligned coordinate: ``o[x]`` is buffer byte x - shift."""

    def __init__(self, aligned_end: int, shift: int, fill=None):
        self.shift = shift
        n = aligned_end - shift
        self.a = fasta_bg(n) if fill is None else np.full(n, fill, np.uint8)

    def put(self, x: int, b) -> None:
        b = np.frombuffer(b, np.uint8) if isinstance(b, (bytes, bytearray)) else np.asarray(b, np.uint8)
        i = x - self.shift
        assert 0 <= i and i + len(b) <= len(self.a), (x, len(b), len(self.a))
        self.a[i:i + len(b)] = b

    def header(self, x: int, length: int, inner_gt: int = 0) -> None:
        """A header line '>' + 'h' * (length - 2) + '\\n' from aligned x, with a '>' every ``inner_gt`` bytes."""
        i = x - self.shift
        self.a[i:i + length] = H_
        if inner_gt:
            self.a[i + inner_gt:i + length - 1:inner_gt] = GT
        self.a[i] = GT
        self.a[i + length - 1] = NL


def _shift_of(i: int) -> int:
    return (5 * i + 3) % 16


# ---------------------------------------------------------------------------------------------- FASTA builders
def build_f_count(events: int, r: int, shift: int) -> np.ndarray:
    """Range r holds ``events // 2`` whole headers ``>h\\n`` and, for an odd count, one header start whose newline
    lies in range r + 1; every other range holds one short header (a non-zero prefix, a line state to carry)."""
    o = _Obj((r + 2) * RANGE + 100, shift)
    for q in range(r + 2):
        if q != r:
            o.put(q * RANGE + 4000, b">id\n")
    x = r * RANGE + 16
    for i in range(events // 2):
        o.put(x + 3 * i, b">h\n")
    if events & 1:
        o.header((r + 1) * RANGE - 8, 17)                  # '>' in range r, '\n' at (r + 1) * RANGE + 8
    return o.a


def boundary_pos(bname: str) -> int:
    """The aligned coordinate of the boundary a last-byte case is built round: a multiple of the named size and of no
    larger one."""
    return {"lane": 2 * RANGE + 3 * ROW + 5 * LANE, "row": 2 * RANGE + 3 * ROW, "buffer": 2 * RANGE + BUF,
            "range": 3 * RANGE, "unit": UNIT, "group": GROUP, "block": BLOCK, "chunk": 2 * RANGE + 5003}[bname]


def boundary_size(bname: str) -> int:
    return {"lane": LANE, "row": ROW, "buffer": BUF, "range": RANGE, "unit": UNIT, "group": GROUP, "block": BLOCK}[bname]


def build_f_last_byte(bname: str, byte: str, where: str, follower: str, shift: int):
    """(data, B): '>' or the newline of a header on the last byte before aligned B (``where`` = "last") or on the
    first byte after it ("first"); a '>' is followed by 'A', by a newline, or by the object's end."""
    if bname == "object":
        B = 3 * RANGE + 777
        o = _Obj(B, shift)
    else:
        B = boundary_pos(bname)
        o = _Obj(B + (1 << 20) if bname == "block" else B + RANGE + 777, shift)
    p = B - 1 if where == "last" else B
    if byte == "gt":
        o.put(p - 3, b"CCC")                               # no newline right before: the line holds no header yet
        o.put(p, b">")
        if follower != "end":
            o.put(p + 1, b"A" if follower == "A" else b"\n")
            o.put(p + 2, b"CG")
    else:
        o.header(p - 19, 20)                               # '>' 19 bytes earlier, its newline on p
        if p + 1 - shift < len(o.a):
            o.put(p + 1, b">z\n")                          # the state after the newline: this one emits
    return o.a, B


def build_f_pending(k: int, shift: int):
    """(data, start, newline): a header line that touches ``k`` ranges (from aligned RANGE - 100 to 100 bytes into
    range k - 1), with a '>' every 1000 bytes (every 90 for k = 2) inside it, then an ordinary header."""
    x0 = RANGE - 100
    length = (k - 2) * RANGE + 201
    o = _Obj((k + 1) * RANGE + 4099, shift)
    o.put(300, b">first\n")
    o.header(x0, length, inner_gt=90 if k == 2 else 1000)
    o.put(x0 + length, b">after\n")
    return o.a, x0 - shift, x0 + length - 1 - shift


def build_f_run(pairs0: int, pairs1: int, shift: int, pending: bool = False) -> np.ndarray:
    """``pairs0`` headers spread evenly over placement block 0 (at most 17 per range), ``pairs1`` in block 1;
    ``pending``: block 0's last header line ends 100 bytes into block 1 (block 1's run starts on an odd slot)."""
    o = _Obj(BLOCK + (64 << 10), shift)
    n0 = pairs0 - (1 if pending else 0)
    if n0:
        step = (BLOCK - 4096) // n0
        assert step >= 900
        for i in range(n0):
            o.put(64 + i * step, b">r\n")
    if pending:
        o.header(BLOCK - 100, 201)
    for i in range(pairs1):
        o.put(BLOCK + 1000 + 5000 * i, b">s\n")
    return o.a


def build_f_chunks(shift: int) -> np.ndarray:
    """Five ranges with a header about every 700 bytes, and '>' / newline bytes round the first range boundary."""
    o = _Obj(5 * RANGE + 333, shift)
    for i, x in enumerate(range(40, 5 * RANGE, 701)):
        o.header(x, 9 + i % 23)
    o.put(RANGE - 2, b"\n>>A")
    o.put(2 * RANGE - 1, b">\n>")
    return o.a


def build_resolve(variant: str, shift: int):
    """(data, buf_len, chunk_hi): a header cut by its chunk's end at ``chunk_hi``; its newline at ``chunk_hi``, at
    ``chunk_hi + 1``, on the buffer's last byte, or absent from the buffer (which ends with the object, or not)."""
    o = _Obj(6000 + shift, shift)
    o.put(100 + shift, b">one\n")
    o.put(900 + shift, b">two\n")
    H, hi = 2000, 2010
    o.a[H:] = H_
    o.a[H] = GT
    n = len(o.a)
    if variant == "nl_at_chunk_hi":
        o.a[hi], buf_len = NL, n
    elif variant == "nl_at_chunk_hi_plus_1":
        o.a[hi + 1], buf_len = NL, n
    elif variant == "nl_on_buffer_last_byte":
        buf_len = 5000
        o.a[buf_len - 1] = NL
    elif variant == "absent_buffer_ends_object":
        buf_len = n
    elif variant == "absent_object_continues":
        buf_len = 5000
        o.a[buf_len] = NL                                  # the byte right after the buffer: not the kernel's to read
    else:
        raise KeyError(variant)
    return o.a, buf_len, hi


RESOLVE_VARIANTS = ("nl_at_chunk_hi", "nl_at_chunk_hi_plus_1", "nl_on_buffer_last_byte", "absent_buffer_ends_object",
                    "absent_object_continues")


def fasta_expect(a: np.ndarray, plan, buf_len: int, pairs_of):
    """What dp_fasta_index must return for ``plan`` over buffer ``a[:buf_len]`` of object ``a``: (pairs (n, 2) uint64,
    chunk_end, pending, unresolved pair indexes).  ``pairs_of(a, chunks)`` is the oracle.  A header cut by its chunk's
    end gets its end from the first newline at or after the chunk end inside the buffer, else the object size if the
    buffer ends with the object, else it stays pending (its end slot is not written)."""
    parts, cend, pending, unresolved, k = [], [], [], [], 0
    for c0, c1 in plan:
        p = pairs_of(a, [(c0, c1)])
        parts.append(p)
        k += len(p)
        cend.append(k)
        pend = -1
        if len(p):
            e = int(p[-1, 1])
            whole = e - 1 < c1 and a[e - 1] == NL
            if not whole and buf_len < len(a) and not np.any(a[c1:buf_len] == NL):
                pend = k - 1
                unresolved.append(k - 1)
        pending.append(pend)
    pairs = np.concatenate(parts) if parts else np.zeros((0, 2), np.uint64)
    return pairs.reshape(-1, 2), cend, pending, unresolved


# ---------------------------------------------------------------------------------------------- newline builders
def build_d_count(count: int, placement: str, r: int, shift: int) -> np.ndarray:
    """Range r holds exactly ``count`` newlines: on its first bytes, on its last bytes, or spread one per lane (the
    remainder on the first lanes' next bytes); every other range a newline about every 997 bytes."""
    o = _Obj((r + 2) * RANGE + 50, shift, fill=X_)
    lo, hi = r * RANGE, (r + 1) * RANGE
    for x in range(max(500, shift), (r + 2) * RANGE + 50, 997):
        if not lo <= x < hi:
            o.put(x, b"\n")
    if placement == "first":
        pos = np.arange(lo, lo + count)
    elif placement == "last":
        pos = np.arange(hi - count, hi)
    else:
        lanes = RANGE // LANE
        per = count // lanes + (np.arange(lanes) < count % lanes)
        pos = np.concatenate([lo + j * LANE + np.arange(per[j]) for j in range(lanes)]) if count else np.zeros(0, int)
    assert len(pos) == count and (count == 0 or pos.min() >= shift)
    o.a[pos.astype(np.int64) - shift] = NL
    return o.a


def build_d_boundary(shift: int) -> np.ndarray:
    """Object bytes [shift, 128 KiB + 300): newlines on object offsets 255, 256, 356, 65535 and 65536 and about every
    4099 bytes."""
    o = _Obj((128 << 10) + 300, shift, fill=X_)
    for x in range(1000, (128 << 10) + 300, 4099):
        o.put(x, b"\n")
    for x in (255, 256, 356, 65535, 65536):
        o.put(x, b"\n")
    return o.a


def build_d_select(shift: int) -> np.ndarray:
    o = _Obj(18 * RANGE, shift, fill=X_)
    for x in range(700, 18 * RANGE, 1499):
        o.put(x, b"\n")
    return o.a


def delim_expect(a: np.ndarray, base: int, ranges, delim: int, k: int, add: int, carry: int, delim_of):
    """(entries uint64, delimiters seen, per-range cumulative counts) of dp_delim_ranges over object bytes
    [base, base + len(a)); ``delim_of(a, begin, end, delim)`` is the oracle (its first result the offsets in a)."""
    parts = [delim_of(a, lo - base, hi - base, delim)[0] + np.uint64(base) for lo, hi in ranges]
    full = np.concatenate(parts)
    ends = np.cumsum([len(p) for p in parts]).tolist()
    sel = (np.arange(len(full), dtype=np.uint64) + np.uint64(carry)) % np.uint64(k) == np.uint64(k - 1)
    return full[sel] + np.uint64(add), len(full), ends


# ---------------------------------------------------------------------------------------------- find builders
FIND_LEN = 3 * ROW + 200


def find_from(m: int, shift: int) -> int:
    """A ``from`` offset whose aligned coordinate is m mod 16."""
    return 48 + ((m - shift) % 16)


def build_find(scenario: str, m: int, shift: int, delim: int) -> np.ndarray:
    """FIND_LEN buffer bytes plus the one byte after them (inside the allocation's padding, never the kernel's to
    report); the filler is never a delimiter."""
    a = np.full(FIND_LEN + 1, X_, np.uint8)
    f = find_from(m, shift)
    step0 = ((f + shift) & ~15) - shift                    # buffer offset of the first 16-byte block wave_find reads
    if scenario == "at_from":
        a[f] = delim
    elif scenario == "before_from":
        a[f - 1] = delim
    elif scenario == "last_byte":
        a[f - 1] = a[FIND_LEN - 1] = delim
    elif scenario == "past_buf_len":
        a[f - 1] = a[FIND_LEN] = delim
    elif scenario == "second_step":
        a[f - 1] = a[step0 + ROW + 100] = a[step0 + 2 * ROW + 100] = delim
    elif scenario == "third_step":
        a[f - 1] = a[step0 + 2 * ROW + 100] = delim
    else:
        raise KeyError(scenario)
    return a


def find_expect(a: np.ndarray, buf_len: int, start: int, delim: int) -> int:
    hit = np.flatnonzero(a[start:buf_len] == delim)
    return start + int(hit[0]) if len(hit) else -1


# ---------------------------------------------------------------------------------------------- the table
def _one(n):
    return [(0, n)]


def _f_count_cases():
    out = []
    for i, ev in enumerate(F_COUNT_EVENTS):
        for j, r in enumerate(F_COUNT_RANGES):
            s = _shift_of(3 * i + j)
            n = (r + 2) * RANGE + 100 - s
            out.append(_case(f"F-count-{ev}-r{r}-s{s}", "fasta", lambda ev=ev, r=r, s=s: build_f_count(ev, r, s),
                             [_one(n)], ("events_in_range", r, ev), s))
    return out


def _f_last_byte_cases():
    out, i = [], 0
    for b in BOUNDARIES:
        combos = [("gt", w, f) for w in ("last", "first") for f in ("A", "nl")] + [("nl", "last", ""), ("nl", "first", "")]
        if b == "object":
            combos = [("gt", "last", "end"), ("nl", "last", "")]
        for byte, where, fol in combos:
            s = _shift_of(i)
            i += 1

            def build(b=b, byte=byte, where=where, fol=fol, s=s):
                return build_f_last_byte(b, byte, where, fol, s)[0]
            if b == "object":
                B = 3 * RANGE + 777
                n = B - s
            else:
                B = boundary_pos(b)
                n = (B + (1 << 20) if b == "block" else B + RANGE + 777) - s
            cut = [(0, B - s), (B - s, n)]
            plans = [_one(n)] if b == "object" else [cut] if b == "chunk" else [_one(n), cut]
            prop = (f"{byte}_{where}_byte_of", b) + ((f"followed_by_{fol}",) if byte == "gt" else ())
            out.append(_case(f"F-last-byte-{b}-{byte}-{where}" + (f"-{fol}" if fol else "") + f"-s{s}", "fasta", build,
                             plans, prop, s, boundary=B))
    return out


def _f_pending_cases():
    out = []
    for i, k in enumerate((2, 17, 1025)):
        s = _shift_of(i + 1)
        n = (k + 1) * RANGE + 4099 - s
        start, nl = RANGE - 100 - s, RANGE - 100 + (k - 2) * RANGE + 200 - s
        mid = (start + nl) // 2
        plans = [_one(n), [(0, mid), (mid, n)], [(0, mid)]]      # whole; cut inside the line; one chunk short
        out.append(_case(f"F-pending-{k}-ranges-s{s}", "fasta", lambda k=k, s=s: build_f_pending(k, s)[0], plans,
                         ("header_spans_ranges", k), s, header=(start, nl), mid=mid))
    return out


def _f_run_cases():
    out = []
    specs = [(p, 3, False) for p in F_RUN_PAIRS] + [(1, 1, False), (1, 1, True), (16384, 0, False), (8193, 0, False)]
    for i, (p0, p1, pend) in enumerate(specs):
        s = _shift_of(i + 2)
        n = BLOCK + (64 << 10) - s
        out.append(_case(f"F-run-{p0}-{p1}" + ("-pending" if pend else "") + f"-s{s}", "fasta",
                         lambda p0=p0, p1=p1, s=s, pend=pend: build_f_run(p0, p1, s, pend), [_one(n)],
                         ("pairs_in_block", 0, p0, 1, p1), s, retry=True, pending_into_block1=pend))
    return out


def _f_chunks_cases():
    out = []
    s = 6
    n = 5 * RANGE + 333 - s

    def build(s=s):
        return build_f_chunks(s)

    def plan_of(cuts):
        cuts = sorted(set(c for c in cuts if 0 < c < n))
        return list(zip([0] + cuts, cuts + [n]))
    rc = [q * RANGE - s + d for q in range(1, 5) for d in (-1, 0, 1)]
    out.append(_case("F-chunks-range-pm1", "fasta", build, [plan_of(rc)], ("cuts_at", RANGE, (-1, 0, 1)), s))
    lc = [q * LANE - s + d for q in (1, 2, 63, 64, 65, 1024, 1025) for d in (-1, 1)]
    out.append(_case("F-chunks-lane-pm1", "fasta", build, [plan_of(lc)], ("cuts_at", LANE, (-1, 1)), s))
    x = RANGE - s                                           # aligned RANGE: lane [RANGE, RANGE + 16) holds ">A.."
    two = [(0, x + 1), (x + 1, x + 6), (x + 6, x + 12), (x + 12, n)]
    three = [(0, x + 1), (x + 1, x + 4), (x + 4, x + 9), (x + 9, x + 15), (x + 15, n)]
    out.append(_case("F-chunks-two-in-a-lane", "fasta", build, [two], ("chunks_in_one_lane", 2), s))
    out.append(_case("F-chunks-three-in-a-lane", "fasta", build, [three], ("chunks_in_one_lane", 3), s))
    g = RANGE - 1 - s                                       # "\n>>A" from aligned RANGE - 2: '>' at RANGE - 1 and RANGE
    for byte, p in (("gt", g), ("nl", g - 1)):
        plan = [(0, p), (p, p + 1), (p + 1, n)]
        out.append(_case(f"F-chunks-one-byte-{byte}", "fasta", build, [plan, [(p, p + 1)]], ("one_byte_chunk", byte), s))
    e = 2 * RANGE + 17
    out.append(_case("F-chunks-empty", "fasta", build, [[(0, 0), (0, e), (e, e), (e, e), (e, n), (n, n)], [(5, 5)]],
                     ("empty_chunks", 4), s))
    for k in range(1, 16):
        out.append(_case(f"F-chunks-first-starts-at-{k}", "fasta", build, [[(k, n)], [(k, RANGE + k), (RANGE + k, n)]],
                         ("first_chunk_start", k), s))
    return out


def _resolve_cases():
    out = []
    for v in RESOLVE_VARIANTS:
        for s in FIND_SHIFTS:
            a, buf_len, hi = build_resolve(v, s)
            out.append(_case(f"R-{v}-s{s}", "fasta", lambda v=v, s=s: build_resolve(v, s)[0],
                             [[(0, hi)], [(0, 950), (950, hi)]], ("resolve", v), s, buf_len=buf_len, chunk_hi=hi))
    return out


def _d_count_cases():
    out, i = [], 0
    for c in D_COUNT_DELIMS:
        for pl in (("all",) if c in (0, 16384) else ("first", "last", "lane")):
            for r in D_COUNT_RANGES:
                s = 0 if r == 0 else _shift_of(i)
                i += 1
                end = (r + 2) * RANGE + 50
                out.append(_case(f"D-count-{c}-{pl}-r{r}-s{s}", "delim", lambda c=c, pl=pl, r=r, s=s: build_d_count(c, pl, r, s),
                                 [[(s, end)]], ("delims_in_range", r, c), s, delim=NL))
    return out


def _d_boundary_cases():
    out = []
    N = (128 << 10) + 300
    # begin / end on the boundary and one byte to either side; a launch inside one 256-byte block (it holds 356)
    launches = [(P, P + d, N) for P in (256, 65536) for d in (-1, 0, 1)] + \
               [(P, None, P + d) for P in (256, 65536) for d in (-1, 0, 1)] + [(256, 266, 456)]
    for i, (P, lo, hi) in enumerate(launches):
        s = (0, 9)[i % 2]
        lo = s if lo is None else lo
        out.append(_case(f"D-boundary-{lo}-{hi}-s{s}", "delim", lambda s=s: build_d_boundary(s), [[(lo, hi)]],
                         ("boundary_launch", P, lo, hi), s, delim=NL))
    return out


def _d_select_cases():
    out = []
    s = 11
    pos = np.arange(700, 18 * RANGE, 1499)
    rng_of = pos // RANGE
    targets = {"first-of-range-3": int(np.flatnonzero(rng_of == 3)[0]), "last-of-range-3": int(np.flatnonzero(rng_of == 3)[-1]),
               "first-of-group-1": int(np.flatnonzero(rng_of == GROUP_RANGES)[0])}
    for k in (2, 3, 4):
        for tn, t in targets.items():
            carry = (k - 1 - t) % k + k
            out.append(_case(f"D-select-k{k}-{tn}", "delim", lambda s=s: build_d_select(s), [[(s, 18 * RANGE)]],
                             ("selects", k, carry, int(pos[t])), s, delim=NL, select=[(k, 0, carry), (k, 1, carry)]))
    k = len(pos) + 3 + 5
    out.append(_case("D-select-k-beyond-count", "delim", lambda s=s: build_d_select(s), [[(s, 18 * RANGE)]],
                     ("selects_none", k, 3, len(pos)), s, delim=NL, select=[(k, 0, 3), (k, 1, 3)]))
    return out


def _d_bytes_cases():
    out = []
    for v in DELIM_BYTES:
        for s in (0, 5):
            out.append(_case(f"D-bytes-0x{v:02X}-s{s}", "delim", every_value_every_position, [[(s, s + 4096)]],
                             ("delim_byte", v), s, delim=v))
    return out


def _find_cases():
    out = []
    for sc in FIND_SCENARIOS:
        for s in FIND_SHIFTS:
            for v in DELIM_BYTES:
                for m in range(16):
                    out.append(_case(f"find-{sc}-s{s}-0x{v:02X}-m{m}", "find",
                                     lambda sc=sc, m=m, s=s, v=v: build_find(sc, m, s, v), [find_from(m, s)],
                                     ("from_mod16", m, sc), s, delim=v, buf_len=FIND_LEN))
    return out


FAMILIES = {"F-count": _f_count_cases, "F-last-byte": _f_last_byte_cases, "F-pending": _f_pending_cases,
            "F-run": _f_run_cases, "F-chunks": _f_chunks_cases, "resolve": _resolve_cases, "D-count": _d_count_cases,
            "D-boundary": _d_boundary_cases, "D-select": _d_select_cases, "D-bytes": _d_bytes_cases, "find": _find_cases}
CASES = {fam: fn() for fam, fn in FAMILIES.items()}
ALL = [c for cs in CASES.values() for c in cs]
assert len({c.name for c in ALL}) == len(ALL), "case names are unique"


def cases_of(kind: str):
    return [c for c in ALL if c.kind == kind]
