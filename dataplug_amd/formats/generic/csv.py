"""CSV format plugin (dataplug/formats/generic/csv.py) with a GPU-built newline index.

``preprocess_csv`` keeps the reference's attributes (``columns``/``dtypes`` from the first 20 lines,
csv.py:20-36) and additionally stores the sorted offsets of every ``'\\n'`` (scanned on the GPUs) at
``<key>.lines`` in the meta bucket (attributes ``num_lines``, ``line_index_key``, ``line_index_dtype``; with
``index_format="auto"`` the u8s form, or u16b for objects with fewer than one newline per 128 bytes).  The meta
object itself stays empty, as in the reference.  The partition strategies produce the reference's
``range_0``/``range_1`` and a ``get()`` with identical output, resolved from the index instead of a
padded Python scan per slice (the reference's formulas: ``_lines.csv_body``).

Opt-in, beyond the reference: ``preprocess(extra_args={"quotechar": '"'})`` also stores the quote-aware record ends
(the ``'\\n'`` outside quoted fields, RFC 4180; built on the GPU by libdpquote.so) as uint64 at ``<key>.records``
(attributes ``record_index_key``, ``num_records``, ``quotechar``), and ``partition_records_num_chunks`` /
``partition_records_chunk_size`` cut only at record ends, so a line break inside a quoted field never splits a row.
``record_index_format="u16b"`` (default ``"u64"``) stores the same record ends in a quarter of the bytes: uint16 low
words at ``<key>.records`` and the 64 KiB block table at ``<key>.records.blocks``, both written by the kernel
(attributes ``record_index_dtype``, ``record_index_blocks_key``, ``record_index_block0``); the strategies read either.
``escapechar`` (with ``quotechar``; for example ``"\\\\"``) is for the dialect that writes a quote inside a field as
``\\"`` (Spark, Hive, MySQL, ``csv.writer(escapechar=..., doublequote=False)``): the byte after an unescaped escape
byte is literal, so an escaped quote does not open or close a field (include/dpquote.h).  ``escape_scope`` "all"
(default; Python's csv module and pandas: the escape works outside quoted fields too, an escaped line break continues
the record) or "quoted" (Spark / univocity: a line break outside a quoted field always ends the record).  The attributes
``escapechar`` and ``escape_scope`` are stored, and ``CSVSlice.get_as_pandas`` parses with the stored dialect.
"""
from __future__ import annotations

import io
import logging
from math import ceil
from typing import TYPE_CHECKING, List, Optional

from ...entities import CloudDataFormat, CloudObjectSlice, PartitioningStrategy
from ...preprocessing.metadata import PreprocessingMetadata
from .._lines import LineIndex, SliceError, csv_body, index_object, records_of, slice_error, snap, store_record_index

if TYPE_CHECKING:
    from ...cloudobject import CloudObject

logger = logging.getLogger(__name__)


def preprocess_csv(cloud_object: "CloudObject", separator: str = ",", line_index: bool = True,
                   index_format: str = "auto", quotechar: Optional[str] = None,
                   record_index_format: str = "u64", escapechar: Optional[str] = None,
                   escape_scope: str = "all") -> PreprocessingMetadata:
    import pandas as pd

    if record_index_format not in ("u64", "u16b"):
        raise ValueError(f"record_index_format must be 'u64' or 'u16b', not {record_index_format!r}")
    if escape_scope not in ("all", "quoted"):
        raise ValueError(f"escape_scope must be 'all' or 'quoted', not {escape_scope!r}")
    if escapechar is not None:
        if quotechar is None:
            raise ValueError("escapechar needs quotechar")
        e = escapechar.encode("utf-8")
        if len(e) != 1 or e == b"\n" or e == quotechar.encode("utf-8"):
            raise ValueError(f"escapechar must be one byte other than the quote and a newline, not {escapechar!r}")

    top = []
    with cloud_object.open("r") as f:
        for _ in range(20):
            top.append(f.readline().strip())
        if quotechar is not None:
            # the sample must end at a record end: read on while it stops inside a quoted field
            while _open_quotes(top, quotechar, escapechar) and len(top) < 4096:
                line = f.readline()
                if not line:
                    break
                top.append(line.strip())
    dialect = {} if quotechar is None else {"quotechar": quotechar}
    if escapechar is not None:
        dialect["escapechar"] = escapechar
    df = pd.read_csv(io.StringIO("\n".join(top)), sep=separator, **dialect)
    attrs = {"columns": df.columns.tolist(), "dtypes": df.dtypes.tolist()}
    if line_index:
        attrs.update(index_object(cloud_object, 0, index_format))
    if quotechar is not None:
        q = quotechar.encode("utf-8")
        if len(q) != 1 or q == b"\n":
            raise ValueError(f"quotechar must be one byte other than a newline, not {quotechar!r}")
        from ...scan import objects as so
        kw = {} if record_index_format == "u64" else {"fmt": record_index_format}
        if escapechar is not None:
            kw.update(escape=escapechar.encode("utf-8")[0], escape_scope=escape_scope)
        attrs.update(store_record_index(cloud_object, so.record_index_object(cloud_object, quote=q[0], **kw),
                                        quotechar, **({} if escapechar is None else
                                                      {"escapechar": escapechar, "escape_scope": escape_scope})))
    return PreprocessingMetadata(attributes=attrs)


def _open_quotes(lines, quotechar: str, escapechar: Optional[str]) -> int:
    """1 iff the sample ``lines`` stop inside a quoted field: the parity of their quotes, the escaped ones left out."""
    if escapechar is None:
        return sum(t.count(quotechar) for t in lines) % 2
    n = esc = 0
    for ch in "\n".join(lines):
        if esc:
            esc = 0
        elif ch == escapechar:
            esc = 1
        elif ch == quotechar:
            n += 1
    return n % 2


@CloudDataFormat(preprocessing_function=preprocess_csv)
class CSV:
    columns: List[str]
    dtypes: List[str]
    num_lines: int
    line_index_key: str


class CSVSlice(CloudObjectSlice):
    def __init__(self, chunk_id, num_chunks, padding, *args, body: Optional[tuple] = None,
                 error: Optional[SliceError] = None, **kwargs):
        self.chunk_id = chunk_id
        self.num_chunks = num_chunks
        self.padding = padding
        self.body = body            # object bytes [start, end) this slice returns
        self.error = error
        super().__init__(*args, **kwargs)

    def get_bytes(self) -> bytes:
        if self.error is not None:
            raise slice_error(self.error)
        co = self.cloud_object
        start, end = self.body
        data = b""
        if end > start:
            data = co.storage.get_object(Bucket=co.path.bucket, Key=co.path.key,
                                         Range=f"bytes={start}-{end - 1}")["Body"].read()
        if self.range_0 != 0:
            data = (",".join(co.attributes.columns) + "\n").encode("utf-8") + data
        return data

    def get(self) -> str:
        return self.get_bytes().decode("utf-8")

    def get_as_pandas(self):
        import pandas as pd
        attrs = self.cloud_object.attributes
        esc = getattr(attrs, "escapechar", None) if attrs is not None else None
        if esc:                                          # the dialect the record index was built for
            return pd.read_csv(io.StringIO(self.get()), quotechar=attrs.quotechar, escapechar=esc)
        return pd.read_csv(io.StringIO(self.get()))


def _slices(cloud_object, chunk_size: int, num_chunks: int, padding: int) -> List[CSVSlice]:
    size = cloud_object.size
    lines = LineIndex.of(cloud_object)
    out = []
    for i in range(num_chunks):
        r0 = chunk_size * i
        r0 = r0 - 1 if r0 > 0 else r0
        r1 = chunk_size * i + chunk_size
        r1 = size if r1 > size else r1 + padding
        try:
            body, err = csv_body(lines, size, r0, r1, i, num_chunks, padding), None
        except SliceError as e:
            body, err = None, e
        out.append(CSVSlice(range_0=r0, range_1=r1, chunk_id=i, num_chunks=num_chunks, padding=padding,
                            body=body, error=err))
    return out


@PartitioningStrategy(dataformat=CSV)
def partition_chunk_size(cloud_object: "CloudObject", chunk_size: int, padding: int = 256) -> List[CSVSlice]:
    """csv.py:112-129."""
    assert chunk_size <= cloud_object.size, "Chunk size must be smaller than the file size"
    return _slices(cloud_object, chunk_size, ceil(cloud_object.size / chunk_size), padding)


@PartitioningStrategy(dataformat=CSV)
def partition_num_chunks(cloud_object: "CloudObject", num_chunks: int, padding: int = 256) -> List[CSVSlice]:
    """csv.py:132-148."""
    return _slices(cloud_object, ceil(cloud_object.size / num_chunks), num_chunks, padding)


def _record_slices(cloud_object, chunk_size: int, num_chunks: int) -> List[CSVSlice]:
    """Slice i = [snap(i * chunk_size), snap((i + 1) * chunk_size)) over the record boundaries (``_lines.snap``):
    the bodies tile the object, each ends at a record end (or the object's end), and may be empty."""
    size = cloud_object.size
    records = records_of(cloud_object)
    cuts = [snap(records, size, min(size, i * chunk_size)) for i in range(num_chunks)] + [size]
    return [CSVSlice(range_0=cuts[i], range_1=cuts[i + 1], chunk_id=i, num_chunks=num_chunks, padding=0,
                     body=(cuts[i], cuts[i + 1])) for i in range(num_chunks)]


@PartitioningStrategy(dataformat=CSV)
def partition_records_chunk_size(cloud_object: "CloudObject", chunk_size: int) -> List[CSVSlice]:
    """Slices of about ``chunk_size`` bytes cut at quote-aware record ends (needs ``quotechar`` at preprocess)."""
    assert 0 < chunk_size <= cloud_object.size, "Chunk size must be positive and at most the file size"
    return _record_slices(cloud_object, chunk_size, ceil(cloud_object.size / chunk_size))


@PartitioningStrategy(dataformat=CSV)
def partition_records_num_chunks(cloud_object: "CloudObject", num_chunks: int) -> List[CSVSlice]:
    """``num_chunks`` slices cut at quote-aware record ends (needs ``quotechar`` at preprocess)."""
    assert num_chunks > 0, "num_chunks must be positive"
    return _record_slices(cloud_object, max(1, ceil(cloud_object.size / num_chunks)), num_chunks)
