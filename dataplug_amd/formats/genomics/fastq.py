"""FASTQ.gz (dataplug/formats/genomics/fastq.py): reads = 4 lines; per-read index from the GPU scan.

Below it, uncompressed FASTQ (``FASTQ``): ``preprocess_fastq`` builds a base-aware read index on the GPU
(include/dpfq.h holds the definition; libdpfq.so) and stores it at ``<key>.fqi`` in the meta bucket: the byte offset
of every ``reads_index_every``-th read and the bases before it, as pairs of little-endian uint64, closed by
(size, bases).  ``partition_reads_strategy`` cuts at equal read counts, ``partition_bases_strategy`` at equal bases
(long-read data, whose read lengths span orders of magnitude), ``fetch_reads`` returns a range of reads.  Only
four-line FASTQ is indexed: wrapped FASTQ raises ``FastqFormatError``.
"""
from __future__ import annotations

from bisect import bisect_left, bisect_right
from math import ceil
from typing import TYPE_CHECKING, List

import numpy as np

from ...entities import CloudDataFormat, CloudObjectSlice, PartitioningStrategy
from ...preprocessing.metadata import PreprocessingMetadata
from ...scan.fastq import FastqFormatError  # noqa: F401  (raised by preprocess_fastq)
from ..compressed.gzipped import GZipText, GZipTextSlice, _get_ranges_from_line_pairs, _line_pairs_lines_per_chunk

if TYPE_CHECKING:
    from ...cloudobject import CloudObject

FASTQGZip = GZipText


def read_pairs(total_lines: int, num_batches: int):
    """1-based [line_0, line_1) per batch (fastq.py:21-40)."""
    if (total_lines % 4) != 0:
        raise Exception("Number of lines does not correspond to FASTQ reads format!")
    num_reads = total_lines // 4
    reads_batch = ceil(num_reads / num_batches)
    rp = [(reads_batch * i, (reads_batch * i) + reads_batch) for i in range(num_batches)]
    lp = [((l0 * 4) + 1, (l1 * 4) + 1) for l0, l1 in rp]
    if lp[-1][1] > total_lines:
        lp[-1] = (lp[-1][0], total_lines + 1)
    return lp


@PartitioningStrategy(FASTQGZip)
def partition_reads_batches(cloud_object: "CloudObject", num_batches: int) -> List[GZipTextSlice]:
    """fastq.py:19-48."""
    lp = read_pairs(int(cloud_object.get_attribute("total_lines")), num_batches)
    ranges = _get_ranges_from_line_pairs(cloud_object, lp)
    return [GZipTextSlice(l0, l1, r0, r1) for (l0, l1), (r0, r1) in zip(lp, ranges)]


@PartitioningStrategy(FASTQGZip)
def partition_sequences_per_chunk(cloud_object, seq_per_chunk: int, strategy: str = "expand") -> List[GZipTextSlice]:
    """fastq.py:51-78 (keeps the reference's swapped zip order, :73-76)."""
    pairs = _line_pairs_lines_per_chunk(int(cloud_object.get_attribute("total_lines")), seq_per_chunk * 4, strategy)
    ranges = _get_ranges_from_line_pairs(cloud_object, pairs)
    return [GZipTextSlice(l0, l1, r0, r1) for (l0, l1), (r0, r1) in zip(ranges, pairs)]


def load_read_index(cloud_object) -> np.ndarray:
    """uint64 end offset (in the inflated stream) of every read, built by preprocess_gzip on the GPU."""
    key = cloud_object.get_attribute("records_key")
    res = cloud_object.storage.get_object(Bucket=cloud_object.meta_path.bucket, Key=key)
    return np.frombuffer(res["Body"].read(), dtype="<u8")


# ------------------------------------------------------------------------------------------ uncompressed FASTQ
FQI_SUFFIX = ".fqi"


def preprocess_fastq(cloud_object: "CloudObject", reads_index_every: int = 64) -> PreprocessingMetadata:
    """Build the read index on the GPUs and store it at ``<key>.fqi``.  On ``FastqFormatError`` nothing is stored."""
    from ...scan import fastq as sfastq
    from ...scan import objects as scan_objects
    from ...version import __version__
    idx = scan_objects.reads_index_object(cloud_object, reads_index_every)
    key = cloud_object.path.key + FQI_SUFFIX
    cloud_object.storage.put_object(Body=sfastq.samples_bytes(idx.samples), Bucket=cloud_object.meta_path.bucket,
                                    Key=key, Metadata={"dataplug": __version__})
    return PreprocessingMetadata(attributes={
        "reads_index_key": key, "reads_index_every": int(reads_index_every), "num_reads": int(idx.num_reads),
        "num_bases": int(idx.num_bases), "min_read_len": int(idx.min_read_len),
        "max_read_len": int(idx.max_read_len)})


@CloudDataFormat(preprocessing_function=preprocess_fastq)
class FASTQ:
    reads_index_key: str
    reads_index_every: int
    num_reads: int
    num_bases: int
    min_read_len: int
    max_read_len: int


def _samples(cloud_object: "CloudObject", j0: int = None, j1: int = None) -> np.ndarray:
    """Entries [j0, j1) of the stored samples (one ranged GET), or all of them."""
    from ...scan import fastq as sfastq
    key = getattr(cloud_object.attributes, "reads_index_key", None)
    if not isinstance(key, str) or not key.endswith(FQI_SUFFIX):         # (unset: the class's annotation)
        raise KeyError("reads index: this object has no read index; preprocess it as formats.genomics.fastq.FASTQ")
    kw = {} if j0 is None else {"Range": f"bytes={16 * j0}-{16 * j1 - 1}"}
    res = cloud_object.storage.get_object(Bucket=cloud_object.meta_path.bucket, Key=key, **kw)
    return sfastq.parse_samples(res["Body"].read())


def load_read_samples(cloud_object: "CloudObject") -> np.ndarray:
    """The stored samples as a structured array with the fields ``offset`` and ``bases``: entry j < S is read
    ``j * reads_index_every``, the last one (size, all bases).  KeyError when the object was not preprocessed as
    ``FASTQ``."""
    return _samples(cloud_object)


class FASTQSlice(CloudObjectSlice):
    """Whole reads: object bytes [range_0, range_1) hold reads [first_read, first_read + num_reads), ``num_bases``
    bases in all."""

    def __init__(self, range_0, range_1, first_read, num_reads, num_bases):
        self.first_read, self.num_reads, self.num_bases = first_read, num_reads, num_bases
        super().__init__(range_0, range_1)

    def get(self) -> str:
        if self.range_1 <= self.range_0:
            return ""
        co = self.cloud_object
        res = co.storage.get_object(Bucket=co.path.bucket, Key=co.path.key,
                                    Range=f"bytes={self.range_0}-{self.range_1 - 1}")
        return res["Body"].read().decode("utf-8")


def _slices(cloud_object, smp: np.ndarray, cuts: List[int]) -> List[FASTQSlice]:
    """One slice per pair of neighbouring sample cuts.  The closing sample S stands for read R, not S * K: a cut there
    (the last one always, an earlier one when the last interval holds a large share of the bases) begins at read R."""
    k, r = int(cloud_object.attributes.reads_index_every), int(cloud_object.attributes.num_reads)
    off, bases = smp["offset"].tolist(), smp["bases"].tolist()
    first = [min(c * k, r) for c in cuts]
    return [FASTQSlice(off[a], off[b], fa, fb - fa, bases[b] - bases[a])
            for a, b, fa, fb in zip(cuts[:-1], cuts[1:], first[:-1], first[1:])]


@PartitioningStrategy(dataformat=FASTQ)
def partition_reads_strategy(cloud_object: "CloudObject", num_chunks: int) -> List[FASTQSlice]:
    """``num_chunks`` slices of whole reads with boundaries at the samples ``(i * S) // num_chunks``: equal read
    counts up to one sample interval.  With more chunks than samples some slices are empty."""
    smp = load_read_samples(cloud_object)
    s = len(smp) - 1
    return _slices(cloud_object, smp, [(i * s) // num_chunks for i in range(num_chunks + 1)])


@PartitioningStrategy(dataformat=FASTQ)
def partition_bases_strategy(cloud_object: "CloudObject", num_chunks: int) -> List[FASTQSlice]:
    """``num_chunks`` slices of whole reads with boundary i at the sample whose cumulative bases are nearest to
    ``i * B / num_chunks`` (the lower sample on a tie; never before the boundary in front): equal work for long-read
    data.  A slice's bases differ from ``B / num_chunks`` by at most the bases of the largest sample interval."""
    smp = load_read_samples(cloud_object)
    s, n = len(smp) - 1, int(num_chunks)
    bases = smp["bases"].tolist()
    cuts = [0]
    for i in range(1, n):
        t = i * bases[-1]                                                # the target, times n
        hi = min(s, bisect_right(bases, t // n))                         # the first sample beyond the target
        lo = bisect_left(bases, bases[max(0, hi - 1)])                   # the lowest of the last ones not beyond it
        j = lo if t - bases[lo] * n <= bases[hi] * n - t else hi
        cuts.append(max(j, cuts[-1]))
    return _slices(cloud_object, smp, cuts + [s])


def fetch_reads(cloud_object: "CloudObject", first: int, count: int) -> bytes:
    """Exactly the reads [first, first + count) as bytes, terminators included: one ranged GET from sample
    ``first // K`` to sample ``ceil((first + count) / K)`` and a walk over its lines.  IndexError out of range."""
    k, r = int(cloud_object.attributes.reads_index_every), int(cloud_object.attributes.num_reads)
    first, count = int(first), int(count)
    if first < 0 or count < 0 or first + count > r:
        raise IndexError(f"reads [{first}, {first + count}) of an object with {r} reads")
    if count == 0:
        return b""
    j0, j1 = first // k, -(-(first + count) // k)
    off = _samples(cloud_object, j0, j1 + 1)["offset"]
    lo, hi = int(off[0]), int(off[-1])
    buf = cloud_object.storage.get_object(Bucket=cloud_object.path.bucket, Key=cloud_object.path.key,
                                          Range=f"bytes={lo}-{hi - 1}")["Body"].read()

    def walk(p: int, lines: int) -> int:
        for _ in range(lines):
            q = buf.find(b"\n", p)
            p = len(buf) if q < 0 else q + 1
        return p
    a = walk(0, 4 * (first - j0 * k))
    return buf[a:walk(a, 4 * count)]
