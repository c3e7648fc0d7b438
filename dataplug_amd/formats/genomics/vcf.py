"""VCF format plugin (dataplug/formats/genomics/vcf.py) with a GPU-built newline index of the body.

``preprocess_vcf`` keeps the reference's header parse and outputs (attributes ``columns``,
``vcf_attributes``, ``body_offset``; meta object = the stripped header lines joined by '\\n',
vcf.py:19-67) and adds the offsets of every '\\n' in ``[body_offset, size)``, scanned on the GPUs in independent
parts (one or more per GPU), stored at ``<key>.lines`` (``index_format="auto"``: the u8s form, or u16b for bodies
with fewer than one newline per 128 bytes; ``_lines.store_line_index``).  ``partition_num_chunks`` gives
the reference's ranges and a ``get()`` with identical output (formulas: ``_lines.vcf_body``).

Opt-in ``extra_args={"pos_index": True}``: a position index (include/dpvpos.h) is built on the GPU -- the POS of every
``pos_index_every``-th body line (uint32 LE) at ``<key>.pos`` and a table of the contig runs at ``<key>.contigs`` in
the meta bucket (attributes ``pos_index_key``, ``pos_index_every``, ``contigs_key``, ``num_contigs``,
``num_body_lines``); ``load_contigs``, ``fetch_region``, ``partition_contigs_strategy`` and
``partition_regions_strategy`` read it.  Without the key every stored byte and attribute is as before.

Opt-in ``extra_args={"pos_index": True, "span_index": True}``: a record-end index (include/dpvspan.h) is built in the
same pass -- the largest rec_end of every ``pos_index_every``-block of body lines (uint32 LE) at ``<key>.ends``
(attributes ``span_index_key``, ``max_span``, ``span_head_ends``), where rec_end is a counting ``END=`` of INFO or
POS + len(REF) - 1.  With it ``region_range``, ``fetch_region`` and ``partition_regions_strategy`` take
``overlap=True`` and return every record whose interval [POS, rec_end] overlaps the region, as ``tabix chr:a-b`` does.
"""
from __future__ import annotations

import logging
import re
from math import ceil
from typing import TYPE_CHECKING, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from ...entities import CloudDataFormat, CloudObjectSlice, PartitioningStrategy
from ...preprocessing.metadata import PreprocessingMetadata
from ...scan.vpos import VcfFormatError  # noqa: F401  (raised by preprocess with pos_index)
from .._lines import LineIndex, SliceError, index_object, slice_error, vcf_body

if TYPE_CHECKING:
    from ...cloudobject import CloudObject

logger = logging.getLogger(__name__)

_DICT_RE = re.compile(r'(\w+)=(".*?"|\w+)')


def parse_vcf_header(f):
    """(header lines, header_metadata, columns, body_offset) from a binary file object at offset 0."""
    header, meta = [], {}

    def line_of():
        raw = f.readline()
        return raw, raw.decode("utf-8").strip()

    raw, line = line_of()
    pos = len(raw)
    assert line.startswith("##fileformat=VCF"), "VCF file does not start with the correct header"
    k, v = line.replace("##", "").split("=")
    meta[k] = v
    header.append(line)
    raw, line = line_of()
    pos += len(raw)
    while line.startswith("##"):
        header.append(line)
        k, v = line.replace("##", "").split("=", 1)
        if "<" in v and ">" in v:
            v = v.strip("<").strip(">")
            d = {a: b.strip('"') for a, b in _DICT_RE.findall(v)}
            meta.setdefault(k, []).append(d)
        else:
            meta[k] = v
        raw, line = line_of()
        pos += len(raw)
    assert line.startswith("#CHROM"), "VCF file does not have the correct header"
    columns = line.replace("#", "").split("\t")
    header.append(line)
    return header, meta, columns, pos


POS_SUFFIX, CONTIGS_SUFFIX, ENDS_SUFFIX = ".pos", ".contigs", ".ends"


def preprocess_vcf(cloud_object: "CloudObject", line_index: bool = True, index_format: str = "auto",
                   pos_index: bool = False, pos_index_every: int = 128,
                   span_index: bool = False) -> PreprocessingMetadata:
    if span_index and not pos_index:
        raise ValueError("span_index needs the position index: pos_index must be True")
    with cloud_object.open("rb") as f:
        header, meta, columns, body_offset = parse_vcf_header(f)
    attrs = {"columns": columns, "vcf_attributes": meta, "body_offset": body_offset}
    if line_index:
        attrs.update(index_object(cloud_object, body_offset, index_format))
    out = PreprocessingMetadata(attributes=attrs, metadata="\n".join(header).encode("utf-8"))
    if pos_index:
        if not line_index:
            raise ValueError("pos_index needs the newline index: line_index must be True")
        _with_pos_index(cloud_object, out, body_offset, pos_index_every, span_index)
    return out


def _with_pos_index(cloud_object: "CloudObject", meta: PreprocessingMetadata, body_offset: int, every: int,
                    span_index: bool = False) -> None:
    """Build and store the position index and add its attributes to ``meta``.  On ``VcfFormatError`` the header, the
    newline index and the attributes are stored as they would be without ``pos_index`` before the error goes on.
    With ``span_index`` the record-end index is built in the same pass and stored at ``<key>.ends``; a "missing REF"
    error goes on once the position index and its attributes are stored, as they would be without ``span_index``."""
    from ...preprocessing.handler import upload_metadata
    from ...scan import objects as scan_objects
    from ...scan import vpos
    from ...version import __version__
    span = None
    try:
        if span_index:
            span = scan_objects.span_index_object(cloud_object, body_offset, every)
            samples, names, rows, n_lines = span[:4]
        else:
            samples, names, rows, n_lines = scan_objects.pos_index_object(cloud_object, body_offset, every)
    except VcfFormatError:
        upload_metadata(cloud_object, meta)
        raise
    st, bucket = cloud_object.storage, cloud_object.meta_path.bucket
    pkey, ckey = cloud_object.path.key + POS_SUFFIX, cloud_object.path.key + CONTIGS_SUFFIX
    user = {"dataplug": __version__}
    st.put_object(Body=np.ascontiguousarray(samples, "<u4").tobytes(), Bucket=bucket, Key=pkey, Metadata=user)
    st.put_object(Body=vpos.contigs_text(names, rows), Bucket=bucket, Key=ckey, Metadata=user)
    meta.attributes = dict(meta.attributes, pos_index_key=pkey, pos_index_every=int(every), contigs_key=ckey,
                           num_contigs=len(names), num_body_lines=int(n_lines))
    if span is None:
        return
    if span.error is not None:
        upload_metadata(cloud_object, meta)
        raise span.error
    ekey = cloud_object.path.key + ENDS_SUFFIX
    st.put_object(Body=np.ascontiguousarray(span.ends, "<u4").tobytes(), Bucket=bucket, Key=ekey, Metadata=user)
    meta.attributes = dict(meta.attributes, span_index_key=ekey, max_span=int(span.max_span),
                           span_head_ends=scan_objects.contig_head_ends(cloud_object, rows, every))


def preprocess_vcf_gz(cloud_object: "CloudObject") -> PreprocessingMetadata:
    raise NotImplementedError("Preprocessing for VCF GZ files is not implemented yet")


@CloudDataFormat(preprocessing_function=preprocess_vcf)
class VCF:
    columns: List[str]
    vcf_attributes: Dict[str, Union[str, List[str], Dict[str, str]]]
    body_offset: int
    num_lines: int
    line_index_key: str
    pos_index_key: str
    pos_index_every: int
    contigs_key: str
    num_contigs: int
    num_body_lines: int
    span_index_key: str
    max_span: int
    span_head_ends: List[int]


class VCFSlice(CloudObjectSlice):
    def __init__(self, chunk_id, num_chunks, padding, *args, body: Optional[tuple] = None,
                 error: Optional[SliceError] = None, bodies: Optional[list] = None, **kwargs):
        self.chunk_id = chunk_id
        self.num_chunks = num_chunks
        self.padding = padding
        self.body = body
        self.bodies = bodies                             # an overlap region's exact byte ranges, in file order
        self.error = error
        super().__init__(*args, **kwargs)

    def get(self) -> str:
        if self.error is not None:
            raise slice_error(self.error)
        co = self.cloud_object
        data = b""
        for start, end in ([self.body] if self.bodies is None else self.bodies):
            if end > start:
                data += co.storage.get_object(Bucket=co.path.bucket, Key=co.path.key,
                                              Range=f"bytes={start}-{end - 1}")["Body"].read()
        header = co.storage.get_object(Bucket=co.meta_path.bucket, Key=co.meta_path.key)["Body"].read()
        return header.decode("utf-8") + "\n" + data.decode("utf-8")


@PartitioningStrategy(dataformat=VCF)
def partition_num_chunks(cloud_object: "CloudObject", num_chunks: int, padding: int = 256) -> List[VCFSlice]:
    """vcf.py:152-173."""
    size = cloud_object.size
    bo = cloud_object["body_offset"]
    chunk_size = ceil((size - bo) / num_chunks)
    lines = LineIndex.of(cloud_object)
    out = []
    for i in range(num_chunks):
        r0 = chunk_size * i + bo
        r1 = r0 + chunk_size - 1
        r0 = r0 - 1 if i != 0 else r0
        r1 = (size - 1) if r1 > size else r1
        try:
            body, err = vcf_body(lines, size, r0, r1, i, num_chunks), None
        except SliceError as e:
            body, err = None, e
        out.append(VCFSlice(range_0=r0, range_1=r1, chunk_id=i, num_chunks=num_chunks, padding=padding,
                            body=body, error=err))
    return out


# ------------------------------------------------------------------------------------------ position index (pos_index)
def load_contigs(cloud_object: "CloudObject"):
    """(names, rows) of the stored contig table: the names as a list of bytes and ``rows`` a structured array with the
    fields first_line, num_lines, offset, end, min_pos, max_pos (``scan.vpos.CONTIG_DTYPE``).  KeyError when the
    object was preprocessed without ``pos_index``."""
    from ...scan import vpos
    key = getattr(cloud_object.attributes, "contigs_key", None)
    if not isinstance(key, str) or not key.endswith(CONTIGS_SUFFIX):     # (unset: the class's annotation)
        raise KeyError("pos_index: this object has no position index; preprocess it with "
                       "extra_args={'pos_index': True}")
    res = cloud_object.storage.get_object(Bucket=cloud_object.meta_path.bucket, Key=key)
    return vpos.parse_contigs(res["Body"].read())


def _contig(cloud_object, chrom):
    names, rows = load_contigs(cloud_object)
    chrom = chrom.encode() if isinstance(chrom, str) else bytes(chrom)
    try:
        return rows[names.index(chrom)]
    except ValueError:
        raise KeyError(f"pos_index: no contig named {chrom!r}") from None


def _samples(cloud_object, j0: int, j1: int) -> np.ndarray:
    """Samples [j0, j1) of the stored ``<key>.pos`` (one ranged GET)."""
    if j1 <= j0:
        return np.zeros(0, np.uint32)
    res = cloud_object.storage.get_object(Bucket=cloud_object.meta_path.bucket,
                                          Key=cloud_object.attributes.pos_index_key,
                                          Range=f"bytes={4 * j0}-{4 * j1 - 1}")
    return np.frombuffer(res["Body"].read(), "<u4")


def _line_offset(lines: LineIndex, body_offset: int, ordinal: int, size: int) -> int:
    """The byte offset of body line ``ordinal`` (the line count itself: the end of the body's last line)."""
    if ordinal == 0:
        return body_offset
    return min(size, lines.value(ordinal - 1) + 1) if ordinal - 1 < lines.count else size


def _window_positions(cloud_object, buf: bytes, w0: int):
    """(byte offsets, POS) of the lines of ``buf`` = object bytes from ``w0``, which starts at a line start."""
    nl = np.flatnonzero(np.frombuffer(buf, np.uint8) == 10)
    starts = np.concatenate([[0], nl + 1])
    starts = starts[starts < len(buf)]
    pos = np.empty(len(starts), np.int64)
    for k, s in enumerate(starts.tolist()):
        try:
            pos[k] = int(buf[s:s + 1024].split(b"\t", 2)[1])
        except (IndexError, ValueError):
            raise ValueError(f"pos_index: the line at byte {w0 + s} of {cloud_object.path.key!r} has no numeric POS: "
                             f"the object does not match its position index (changed after preprocess?)") from None
    return starts + w0, pos


def region_range(cloud_object: "CloudObject", chrom, start: Optional[int] = None, end: Optional[int] = None,
                 lines: Optional[LineIndex] = None, fetch: bool = False, overlap: bool = False):
    """(first byte, one past the last byte, candidate byte range, candidate bytes or None) of the lines of contig
    ``chrom`` with start <= POS <= end.  The candidate lines [a, b) come from the samples
    (``scan.vpos.candidate_lines``) and their byte range from the newline index.  Only the lines of the first and of
    the last sample interval of the candidates are parsed: the first line with POS >= start lies in [a, a + K] and
    the first with POS > end in [b - K, b).  A side that is open is the contig's own bound and is not parsed, so an
    open region reads nothing of the object.  ``fetch``: one ranged GET of the whole candidate range, returned and
    used for the two windows; otherwise each window is a ranged GET of its own.

    ``overlap`` (needs the record-end index, ``span_index``): a fifth entry is added, the records in front of that
    range whose interval [POS, rec_end] reaches ``start`` -- a list of (first byte, one past the last byte, bytes) in
    file order, adjacent lines joined; see ``_overlap_before``.  The four entries in front are the same as without."""
    if not overlap:
        return _region(cloud_object, chrom, start, end, lines, fetch)[:4]
    max_span = _span_attrs(cloud_object)[1]
    out = _region(cloud_object, chrom, start, end, lines, fetch)
    first, row, lines = out[4:]
    if start is None or max_span == 0:
        return out[:4] + ([],)
    if end is not None and start > end:                               # an inverted region has no first line of its own
        first, row, lines = _region(cloud_object, chrom, start, None, lines, False)[4:]
    heads = getattr(cloud_object.attributes, "span_head_ends", None)
    names = load_contigs(cloud_object)[0]
    k = names.index(chrom.encode() if isinstance(chrom, str) else bytes(chrom))
    head = int(heads[k]) if isinstance(heads, (list, tuple)) and k < len(heads) else None
    have = (out[2][0], out[3]) if out[3] and not (end is not None and start > end) else None
    return out[:4] + (_overlap_before(cloud_object, row, first, start, end, lines, head, have),)


def _span_attrs(cloud_object):
    """(key, max_span) of the stored record-end index; KeyError when the object was preprocessed without it."""
    key = getattr(cloud_object.attributes, "span_index_key", None)
    if not isinstance(key, str) or not key.endswith(ENDS_SUFFIX):     # (unset: the class's annotation)
        raise KeyError("span_index: this object has no record-end index; preprocess it with "
                       "extra_args={'pos_index': True, 'span_index': True}")
    return key, int(cloud_object.attributes.max_span)


def _overlap_before(cloud_object, row, first: int, start: int, end: Optional[int], lines: Optional[LineIndex],
                    head_end: Optional[int] = None, have: Optional[tuple] = None):
    """The records of the contig ``row`` in front of body line ``first`` (the first with POS >= start) whose rec_end is
    at least ``start`` (and whose POS is at most ``end``): [(first byte, one past the last byte, bytes)], in file
    order, adjacent lines joined.  One ranged GET reads the slots of ``<key>.ends`` that cover those lines;
    ``scan.vspan.blocks_before`` keeps the K-blocks whose slot reaches ``start`` and the partial block at ``first``; the
    kept blocks' bytes are fetched, adjacent blocks in one GET, and every line of them goes through the definition
    (``scan.vspan.rec_end``).  ``head_end``: the contig's own largest rec_end inside its first K-block when that block
    begins in the contig before (attribute ``span_head_ends``); it stands in for that block's slot, which also covers
    the other contig's lines.  ``have``: (first byte, bytes) of object bytes the caller holds already -- the candidate
    range of ``fetch=True``, which begins with the boundary block -- so that what lies in them is not fetched again."""
    from ...scan import vspan
    l0 = int(row["first_line"])
    if first <= l0:
        return []
    every = int(cloud_object.attributes.pos_index_every)
    size, bo = cloud_object.size, int(cloud_object["body_offset"])
    j0, j1 = l0 // every, (first - 1) // every + 1
    res = cloud_object.storage.get_object(Bucket=cloud_object.meta_path.bucket, Key=_span_attrs(cloud_object)[0],
                                          Range=f"bytes={4 * j0}-{4 * j1 - 1}")
    slots = np.frombuffer(res["Body"].read(), "<u4")
    if head_end is not None and l0 % every:
        slots = slots.copy()
        slots[0] = head_end
    lines = lines or LineIndex.of(cloud_object)
    out = []
    for x, y in vspan.blocks_before(slots, j0, every, l0, first, start):
        b0 = int(row["offset"]) if x == l0 else _line_offset(lines, bo, x, size)
        b1 = _line_offset(lines, bo, y, size)
        held = b""
        g1 = b1
        if have is not None and have[0] < b1 <= have[0] + len(have[1]):
            g1 = max(b0, have[0])
            held = have[1][g1 - have[0]:b1 - have[0]]
        buf = held
        if g1 > b0:
            buf = cloud_object.storage.get_object(Bucket=cloud_object.path.bucket, Key=cloud_object.path.key,
                                                  Range=f"bytes={b0}-{g1 - 1}")["Body"].read() + held
        offs, pos = _window_positions(cloud_object, buf, b0)
        bounds = offs.tolist() + [b1]
        for k, p in enumerate(pos.tolist()):
            s, e = bounds[k] - b0, bounds[k + 1] - b0
            if (end is None or p <= end) and vspan.rec_end(buf[s:e].rstrip(b"\n"), p)[0] >= start:
                if out and out[-1][1] == b0 + s:
                    out[-1] = (out[-1][0], b0 + e, out[-1][2] + buf[s:e])
                else:
                    out.append((b0 + s, b0 + e, buf[s:e]))
    return out


def _region(cloud_object: "CloudObject", chrom, start, end, lines, fetch):
    """``region_range``'s four entries, then the ordinal of the first line with POS >= start (None without a start),
    the contig's row and the line index if one was loaded."""
    from ...scan import vpos
    row = _contig(cloud_object, chrom)
    size, bo = cloud_object.size, int(cloud_object["body_offset"])
    every = int(cloud_object.attributes.pos_index_every)
    l0, l1 = int(row["first_line"]), int(row["first_line"]) + int(row["num_lines"])
    a, b = l0, l1
    if start is not None or end is not None:
        j0, j1 = -(-l0 // every), -(-l1 // every)                     # the samples whose ordinals lie in [l0, l1)
        a, b = vpos.candidate_lines(_samples(cloud_object, j0, j1), j0, every, l0, l1, start, end)
    if a == l0 and b == l1:
        c0, c1 = int(row["offset"]), int(row["end"])
    else:
        lines = lines or LineIndex.of(cloud_object)
        c0, c1 = _line_offset(lines, bo, a, size), _line_offset(lines, bo, b, size)
    if c1 <= c0:
        return c0, c0, (c0, c0), b"" if fetch else None, None if start is None else a, row, lines
    get = lambda x, y: cloud_object.storage.get_object(Bucket=cloud_object.path.bucket, Key=cloud_object.path.key,
                                                       Range=f"bytes={x}-{y - 1}")["Body"].read()
    raw = get(c0, c1) if fetch else None

    def window(i0, i1):
        """The lines [i0, i1) of the candidates: (byte offsets, POS, the window's end)."""
        nonlocal lines
        if i0 == a and i1 == b:
            w0, w1 = c0, c1
        else:
            lines = lines or LineIndex.of(cloud_object)
            w0 = c0 if i0 == a else _line_offset(lines, bo, i0, size)
            w1 = c1 if i1 == b else _line_offset(lines, bo, i1, size)
        buf = raw[w0 - c0:w1 - c0] if raw is not None else get(w0, w1)
        return _window_positions(cloud_object, buf, w0) + (w1,)

    r0, r1 = c0, c1
    first = None
    if start is not None:
        offs, pos, w1 = window(a, min(b, a + every + 1))
        k = int(np.searchsorted(pos, start, "left"))
        r0 = int(offs[k]) if k < len(offs) else w1
        first = a + k
    if end is not None:
        offs, pos, w1 = window(max(a, b - every), b)
        k = int(np.searchsorted(pos, end, "right"))
        r1 = int(offs[k]) if k < len(offs) else w1
    if r1 <= r0:
        return c0, c0, (c0, c1), raw, first, row, lines
    return r0, r1, (c0, c1), raw, first, row, lines


def fetch_region(cloud_object: "CloudObject", chrom, start: Optional[int] = None, end: Optional[int] = None,
                 overlap: bool = False) -> bytes:
    """The lines of contig ``chrom`` that match the region, in file order, each with its terminator.  Coordinates are
    1-based and inclusive, as in ``tabix chr:start-end``; None is open on that side.  An unknown contig raises
    KeyError.

    ``overlap=False`` (the default): the lines with start <= POS <= end.  The test is on POS alone: a record that
    overlaps the region only through the length of REF or an ``END=`` tag is not returned.  One ranged GET fetches the
    candidate lines, which are cut to the exact ones on the host.

    ``overlap=True``: every record whose interval [POS, rec_end] overlaps the region -- rec_end >= start and
    POS <= end -- as ``tabix`` returns them; rec_end is a counting ``END=`` of INFO, else POS + len(REF) - 1
    (include/dpvspan.h).  Needs the record-end index (``extra_args={'pos_index': True, 'span_index': True}``; KeyError
    without it).  The records in front of the POS range are found through ``<key>.ends``: only the K-blocks whose
    largest rec_end reaches ``start`` are fetched.  With ``max_span`` 0, or without a ``start``, the answer is the
    POS-only one."""
    if overlap:
        r0, r1, (c0, _), raw, before = region_range(cloud_object, chrom, start, end, fetch=True, overlap=True)
        return b"".join(x[2] for x in before) + raw[r0 - c0:r1 - c0]
    r0, r1, (c0, _), raw = region_range(cloud_object, chrom, start, end, fetch=True)
    return raw[r0 - c0:r1 - c0]


@PartitioningStrategy(dataformat=VCF)
def partition_contigs_strategy(cloud_object: "CloudObject") -> List[VCFSlice]:
    """One slice per contig run, in file order: ``get()`` returns the header plus that contig's lines."""
    names, rows = load_contigs(cloud_object)
    n = len(rows)
    return [VCFSlice(range_0=int(r["offset"]), range_1=int(r["end"]), chunk_id=i, num_chunks=n, padding=0,
                     body=(int(r["offset"]), int(r["end"]))) for i, r in enumerate(rows)]


@PartitioningStrategy(dataformat=VCF)
def partition_regions_strategy(cloud_object: "CloudObject", regions: Sequence[tuple],
                               overlap: bool = False) -> List[VCFSlice]:
    """One slice per region ``(chrom, start, end)`` (1-based, inclusive, None open; the test is on POS alone): its
    body is the tight byte range of the matching lines, empty for a region without any.  Per region at most two
    sample intervals of lines are read from the object; an open side reads none.

    ``overlap=True`` (needs the record-end index): the test is rec_end >= start and POS <= end, as in
    ``fetch_region``; a slice carries ``bodies``, the exact byte ranges of its records in file order with adjacent
    lines joined, and ``get()`` returns the header plus those ranges."""
    lines = LineIndex.of(cloud_object)
    out = []
    for i, (chrom, start, end) in enumerate(regions):
        if overlap:
            r0, r1, _, _, before = region_range(cloud_object, chrom, start, end, lines=lines, overlap=True)
            bodies = [(x, y) for x, y, _ in before]
            if r1 > r0:
                if bodies and bodies[-1][1] == r0:
                    bodies[-1] = (bodies[-1][0], r1)
                else:
                    bodies.append((r0, r1))
            lo, hi = (bodies[0][0], bodies[-1][1]) if bodies else (r0, r0)
            out.append(VCFSlice(range_0=lo, range_1=hi, chunk_id=i, num_chunks=len(regions), padding=0,
                                body=(lo, hi), bodies=bodies))
            continue
        r0, r1 = region_range(cloud_object, chrom, start, end, lines=lines)[:2]
        out.append(VCFSlice(range_0=r0, range_1=r1, chunk_id=i, num_chunks=len(regions), padding=0, body=(r0, r1)))
    return out
