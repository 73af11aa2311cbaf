"""Host mirror of the read realigner over the C ABI (include/dvhip.h, "read realigner").

  FastPassAligner          deepvariant/realigner/fast_pass_aligner.h (class FastPassAligner)
  realign_reads_to_haplotype   deepvariant/alt_aligned_pileup_lib.cc:278-313
  local_align              deepvariant/realigner/ssw.h (Aligner::SetReferenceSequence + Align)

All computation is native (deepvariant_amd/csrc/fast_pass_aligner.cpp, local_align.cpp); this
module only marshals strings and turns results back into dv_types reads.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

from deepvariant_amd import _lib
from deepvariant_amd import dv_types as T

K_REF_ALIGN_MARGIN = 0    # alt_aligned_pileup_lib.cc:62 kRefAlignMargin (the window realigner's is 20)

BUILD_INDEX, INIT_LOCAL_ALIGNER, ALIGN_HAPLOTYPES, POSITION_MAPS, LOCAL_ALIGN_READS, SCORE_THRESHOLD = range(6)
ALIGN_IN_PHASES = 6     # test hook of dv_aligner_align_reads (include/dvhip.h): arg 1 in phases, 2 with the fast pass split off


def _strings(items: Sequence[str]):
  arr = (C.c_char_p * max(len(items), 1))()
  for i, s in enumerate(items):
    arr[i] = s.encode() if isinstance(s, str) else bytes(s)
  return arr


class ReadAlignment:
  """ReadAlignment (fast_pass_aligner.h:104-128); position None = kNotAligned."""

  def __init__(self, position=None, cigar='', score=0):
    self.position, self.cigar, self.score = position, cigar, score

  def __eq__(self, other):
    return (self.position, self.cigar, self.score) == (other.position, other.cigar, other.score)

  def __repr__(self):
    return 'ReadAlignment(%r, %r, %r)' % (self.position, self.cigar, self.score)


def _read_alignment(raw: _lib.DvReadAlignment) -> ReadAlignment:
  return ReadAlignment(None if raw.position < 0 else raw.position, raw.cigar.decode(), raw.score)


class FastPassAligner:
  def __init__(self, match=0, mismatch=0, gap_open=0, gap_extend=0, kmer_size=0, read_size=0,
               max_num_of_mismatches=0, realignment_similarity_threshold=0.0, force_alignment=False,
               normalize_reads=False, ref_prefix_len=0, ref_suffix_len=0):
    opt = _lib.DvAlignerOptions(match, mismatch, gap_open, gap_extend, kmer_size, read_size,
                                max_num_of_mismatches, realignment_similarity_threshold,
                                int(force_alignment), int(normalize_reads), ref_prefix_len, ref_suffix_len)
    self._h = C.c_void_p()
    _lib.check(_lib.lib().dv_aligner_create(C.byref(opt), C.byref(self._h)))
    self._n_reads = 0

  def __del__(self):
    if getattr(self, '_h', None):
      _lib.lib().dv_aligner_destroy(self._h)
      self._h = None

  def set_reference(self, reference: str, ref_start: int = 0):
    _lib.check(_lib.lib().dv_aligner_set_reference(self._h, reference.encode(), ref_start))

  def set_haplotypes(self, haplotypes: Sequence[str]):
    _lib.check(_lib.lib().dv_aligner_set_haplotypes(self._h, len(haplotypes), _strings(haplotypes)))

  def set_reads(self, reads: Sequence[str]):
    self._n_reads = len(reads)
    _lib.check(_lib.lib().dv_aligner_set_reads(self._h, len(reads), _strings(reads)))

  def stage(self, which: int, arg: int = 0):
    _lib.check(_lib.lib().dv_aligner_stage(self._h, which, arg))

  def fast_align_reads_to_haplotype(self, haplotype: str, haplotype_score: int = 0):
    out = (_lib.DvReadAlignment * max(self._n_reads, 1))()
    score = C.c_int32(haplotype_score)
    _lib.check(_lib.lib().dv_aligner_fast_align(self._h, haplotype.encode(), C.byref(score), out))
    return score.value, [_read_alignment(out[i]) for i in range(self._n_reads)]

  def haplotype_alignment(self, k: int):
    """-> dict(haplotype_index, haplotype_score, ref_pos, is_reference, cigar)."""
    idx, score, is_ref = C.c_int32(), C.c_int32(), C.c_int32()
    pos = C.c_int64()
    buf = C.create_string_buffer(4096)
    _lib.check(_lib.lib().dv_aligner_haplotype_info(self._h, k, C.byref(idx), C.byref(score), C.byref(pos),
                                                    C.byref(is_ref), buf, len(buf)))
    return dict(haplotype_index=idx.value, haplotype_score=score.value, ref_pos=pos.value,
                is_reference=bool(is_ref.value), cigar=buf.value.decode())

  def read_alignment(self, k: int, read: int) -> ReadAlignment:
    raw = _lib.DvReadAlignment()
    _lib.check(_lib.lib().dv_aligner_read_alignment(self._h, k, read, C.byref(raw)))
    return _read_alignment(raw)

  def calculate_read_to_ref_alignment(self, read_index: int, position: int, read_cigar: str,
                                      haplotype_cigar: str) -> str:
    buf = C.create_string_buffer(4096)
    _lib.check(_lib.lib().dv_aligner_merge_alignment(self._h, read_index, position, read_cigar.encode(),
                                                     haplotype_cigar.encode(), buf, len(buf)))
    return buf.value.decode()

  def is_alignment_normalized(self, cigar: str, ref_offset: int, read: str) -> bool:
    r = _lib.lib().dv_aligner_is_normalized(self._h, cigar.encode(), ref_offset, read.encode())
    if r < 0:
      _lib.check(r)
    return bool(r)

  def score_threshold(self) -> int:
    return _lib.lib().dv_aligner_score_threshold(self._h)

  def kmer_occurrences(self, kmer: str) -> List[Tuple[int, int]]:
    cap = 4096
    reads, offs = (C.c_int32 * cap)(), (C.c_int32 * cap)()
    n = _lib.lib().dv_aligner_kmer_occurrences(self._h, kmer.encode(), cap, reads, offs)
    if n < 0:
      _lib.check(n)
    return [(reads[i], offs[i]) for i in range(min(n, cap))]

  def index_size(self) -> int:
    return _lib.lib().dv_aligner_kmer_occurrences(self._h, b'', 0, None, None)

  def align_reads(self, sequences: Sequence[str]):
    """AlignReads on bare sequences -> [(status, position, [(op, length), ...])]."""
    n = len(sequences)
    self._n_reads += n
    out = (_lib.DvRealignedRead * max(n, 1))()
    words = C.POINTER(C.c_uint32)()
    _lib.check(_lib.lib().dv_aligner_align_reads(self._h, n, _strings(sequences), out, C.byref(words)))
    res = []
    for i in range(n):
      cig = [(words[out[i].cigar_off + k] & 15, words[out[i].cigar_off + k] >> 4) for k in range(out[i].n_cigar)]
      res.append((out[i].status, out[i].position, cig))
    return res

  def align_reads_arrays(self, sequences: Sequence):
    """AlignReads on bare sequences, results as arrays (the table path of the realigner):
    -> (status int32[n], position int64[n], cigar_off int64[n + 1], CIGAR words uint32[...] in the
    packed tables' encoding); status as in `align_reads`."""
    import numpy as np
    n = len(sequences)
    self._n_reads += n
    out = (_lib.DvRealignedRead * max(n, 1))()
    words = C.POINTER(C.c_uint32)()
    _lib.check(_lib.lib().dv_aligner_align_reads(self._h, n, _strings(sequences), out, C.byref(words)))
    rec = np.frombuffer(out, dtype=np.dtype([('status', '<i4'), ('n_cigar', '<i4'), ('position', '<i8'),
                                             ('cigar_off', '<u4'), ('reserved', '<u4')]), count=max(n, 1))[:n]
    off = np.zeros(n + 1, np.int64)
    np.cumsum(rec['n_cigar'], out=off[1:])
    total = int(off[-1])
    w = np.ctypeslib.as_array(words, shape=(total,)).copy() if total else np.zeros(0, np.uint32)
    return rec['status'].copy(), rec['position'].copy(), off, w

  def realign_reads(self, reads: Sequence) -> List[Optional[T.Read]]:
    """FastPassAligner::AlignReads on Read objects (fast_pass_aligner.cc:183-232, :510-590):
    per input read the read with its new alignment, the unchanged read (no better alignment,
    or the merged CIGAR was rejected), or None where the reference returns an empty Read
    (force_alignment and nothing found)."""
    out = []
    for read, (status, position, cigar) in zip(reads, self.align_reads([r.aligned_sequence for r in reads])):
      if status == 2:
        out.append(None)
      elif status == 0:
        out.append(read)
      else:
        out.append(with_alignment(read, position, cigar))
    return out


def with_alignment(read, position: int, cigar) -> T.Read:
  """A copy of `read` whose alignment start and CIGAR are replaced (RealignReadsToReference,
  fast_pass_aligner.cc:510-590: everything else is merged over from the input read)."""
  p = read.alignment.position
  return T.Read(
      fragment_name=read.fragment_name, read_number=read.read_number,
      number_reads=read.number_reads, fragment_length=read.fragment_length,
      proper_placement=read.proper_placement, duplicate_fragment=read.duplicate_fragment,
      failed_vendor_quality_checks=read.failed_vendor_quality_checks,
      secondary_alignment=read.secondary_alignment,
      supplementary_alignment=read.supplementary_alignment,
      aligned_sequence=read.aligned_sequence, aligned_quality=read.aligned_quality,
      alignment=T.LinearAlignment(position=T.Position(p.reference_name, position, p.reverse_strand),
                                  mapping_quality=read.alignment.mapping_quality,
                                  cigar=[T.CigarUnit(op, ln) for op, ln in cigar]),
      info=dict(read.info), base_modifications=dict(read.base_modifications))


def positions_map(cigar: str, haplotype_size: int) -> List[int]:
  out = (C.c_int32 * max(haplotype_size, 1))()
  _lib.check(_lib.lib().dv_positions_map(cigar.encode(), haplotype_size, out))
  return list(out[:haplotype_size])


def merge_cigar_op(cigar: str, op: str, length: int, read_len: int) -> str:
  buf = C.create_string_buffer(cigar.encode(), 4096)
  _lib.check(_lib.lib().dv_merge_cigar_op(buf, len(buf), op.encode(), length, read_len))
  return buf.value.decode()


def local_align(reference: str, query: str, match=2, mismatch=2, gap_open=3, gap_extend=1):
  """One local alignment; defaults are libssw's Aligner() defaults."""
  out = _lib.DvLocalAlignment()
  _lib.check(_lib.lib().dv_local_align(reference.encode(), query.encode(), match, mismatch, gap_open,
                                       gap_extend, C.byref(out)))
  return out


def local_align_many(reference: str, queries: Sequence[str], match=2, mismatch=2, gap_open=3, gap_extend=1):
  """`local_align` of every query against one reference through the 16-lane batch path;
  an entry is None where local_align would raise."""
  n = len(queries)
  out = (_lib.DvLocalAlignment * max(n, 1))()
  _lib.check(_lib.lib().dv_local_align_many(reference.encode(), n, _strings(queries), match, mismatch, gap_open,
                                            gap_extend, out))
  return [None if out[k].score < 0 else out[k] for k in range(n)]


def local_align_band(reference: str, query: str, match=2, mismatch=2, gap_open=3, gap_extend=1) -> Tuple[int, int]:
  """-> (band, runs) of `local_align(reference, query)`'s CIGAR: the band the banded re-alignment ended with and
  the number of M/I/D runs, (0, 0) where there is no CIGAR.  Host only.  The device traces a swept pair back
  itself exactly when band <= _lib.DV_LOCAL_ALIGN_DEVICE_MAX_BAND and runs <= _lib.DV_LOCAL_ALIGN_DEVICE_MAX_RUNS."""
  band, runs = C.c_int32(), C.c_int32()
  _lib.check(_lib.lib().dv_local_align_band(reference.encode(), query.encode(), match, mismatch, gap_open,
                                            gap_extend, C.byref(band), C.byref(runs)))
  return band.value, runs.value


def local_align_pairs_device(sequences: Sequence[str], pairs: Sequence[Tuple[int, int]], scoring=(2, 2, 3, 1),
                             stream: int = 0, with_stats: bool = False, with_traceback_stats: bool = False):
  """`local_align(sequences[r], sequences[q])` for every (r, q) of `pairs`, with the two Smith-Waterman
  sweeps of all pairs in ONE kernel launch (csrc/local_align.hip).  With DV_REALIGN_DEVICE_TRACEBACK=1 the
  same launch traces the alignments back and the host writes the CIGAR text from the device's M/I/D runs;
  otherwise the host's banded re-alignment builds the CIGARs from the corner points.
  `scoring` = (match, mismatch, gap_open, gap_extend).  An entry is None where local_align would
  raise; pairs beyond the kernel's limits (_lib.DV_LOCAL_ALIGN_DEVICE_MAX_*) are aligned by the host
  code inside the call.  There is no CPU fallback: without a GPU this raises DV_ERR_NO_DEVICE.
  with_stats: -> (alignments, _lib.DvRealignDeviceStats of this call);
  with_traceback_stats: _lib.DvRealignTracebackStats of this call is appended to that."""
  import numpy as np
  raw = [s.encode() if isinstance(s, str) else bytes(s) for s in sequences]
  off = np.zeros(len(raw) + 1, np.int64)
  np.cumsum([len(b) for b in raw], out=off[1:])
  bases = b''.join(raw)
  ref = np.ascontiguousarray([p[0] for p in pairs], np.int32)
  query = np.ascontiguousarray([p[1] for p in pairs], np.int32)
  n = len(ref)
  out = (_lib.DvLocalAlignment * max(n, 1))()
  match, mismatch, gap_open, gap_extend = scoring
  _lib.check(_lib.lib().dv_local_align_pairs_device(len(raw), bases, off.ctypes.data, n, ref.ctypes.data,
                                                    query.ctypes.data, match, mismatch, gap_open, gap_extend, out,
                                                    stream or None))
  res = [None if out[k].score < 0 else out[k] for k in range(n)]
  if not with_stats and not with_traceback_stats:
    return res
  ret = (res,)
  if with_stats:
    stats = _lib.DvRealignDeviceStats()
    _lib.check(_lib.lib().dv_local_align_device_last_stats(C.byref(stats)))
    ret += (stats,)
  if with_traceback_stats:
    traceback = _lib.DvRealignTracebackStats()
    _lib.check(_lib.lib().dv_local_align_device_last_traceback_stats(C.byref(traceback)))
    ret += (traceback,)
  return ret


def _fast_pass(entry, windows, options, stream):
  import numpy as np
  raw, descs = [], (_lib.DvFastPassWindow * max(len(windows), 1))()
  as_bytes = lambda s: s.encode('latin-1') if isinstance(s, str) else bytes(s)      # noqa: E731
  shapes = []
  for d, w in zip(descs, windows):
    reads, haplotypes = [as_bytes(r) for r in w['reads']], [as_bytes(h) for h in w['haplotypes']]
    d.first_read, d.n_reads = len(raw), len(reads)
    raw += reads
    d.first_haplotype, d.n_haplotypes = len(raw), len(haplotypes)
    raw += haplotypes
    d.reference = -1
    if w.get('reference') is not None:
      d.reference = len(raw)
      raw.append(as_bytes(w['reference']))
    d.ref_prefix_len, d.ref_suffix_len = w.get('ref_prefix_len', 0), w.get('ref_suffix_len', 0)
    shapes.append((len(haplotypes), len(reads)))
  off = np.zeros(len(raw) + 1, np.int64)
  np.cumsum([len(b) for b in raw], out=off[1:])
  table = b''.join(raw)
  n_haps = sum(h for h, _ in shapes)
  n_rows = sum(h * r for h, r in shapes)
  hap_score, hap_discarded = np.zeros(max(n_haps, 1), np.int32), np.zeros(max(n_haps, 1), np.int32)
  position, score = np.zeros(max(n_rows, 1), np.int32), np.zeros(max(n_rows, 1), np.int32)
  opt = _lib.DvAlignerOptions()
  for name, value in (options or {}).items():
    setattr(opt, name, value)
  _lib.check(entry(len(raw), table, off.ctypes.data, len(windows), descs, C.byref(opt), stream or None,
                   hap_score.ctypes.data, hap_discarded.ctypes.data, position.ctypes.data, score.ctypes.data))
  out, h0, r0 = [], 0, 0
  for n_h, n_r in shapes:
    rows = slice(r0, r0 + n_h * n_r)
    out.append(dict(haplotype_score=hap_score[h0:h0 + n_h].copy(), haplotype_discarded=hap_discarded[h0:h0 + n_h].copy(),
                    read_position=position[rows].reshape(n_h, n_r).copy(), read_score=score[rows].reshape(n_h, n_r).copy()))
    h0, r0 = h0 + n_h, r0 + n_h * n_r
  return out


def fast_pass_batch(windows: Sequence[dict], options: Optional[dict] = None):
  """FastPassAligner's fast pass (FastAlignReadsToHaplotype) for every haplotype of every window, host code.
  A window is dict(reads=[...], haplotypes=[...], reference=str or None, ref_prefix_len=0, ref_suffix_len=0); reads
  are upper-cased by the call.  `options`: fields of dv_aligner_options (match, mismatch, kmer_size,
  max_num_of_mismatches; 0 or absent keeps the class default).  -> per window dict(haplotype_score int32[h],
  haplotype_discarded int32[h], read_position int32[h, r] (-1: not aligned), read_score int32[h, r])."""
  return _fast_pass(_lib.lib().dv_fast_pass_batch, windows, options, 0)


def fast_pass_batch_device(windows: Sequence[dict], options: Optional[dict] = None, stream: int = 0,
                           with_stats: bool = False):
  """`fast_pass_batch` with every (window, haplotype) in ONE kernel launch (csrc/fast_pass.hip); identical arrays.
  A haplotype longer than _lib.DV_FAST_PASS_DEVICE_MAX_HAPLOTYPE is run by the host code inside the call.  There is
  no CPU fallback: without a GPU this raises DV_ERR_NO_DEVICE.  with_stats: -> (windows, _lib.DvFastPassStats)."""
  res = _fast_pass(_lib.lib().dv_fast_pass_batch_device, windows, options, stream)
  if not with_stats:
    return res
  stats = _lib.DvFastPassStats()
  _lib.check(_lib.lib().dv_fast_pass_device_last_stats(C.byref(stats)))
  return res, stats


def _align_windows(entry, windows, options, stream):
  import numpy as np
  raw, descs = [], (_lib.DvAlignWindow * max(len(windows), 1))()
  as_bytes = lambda s: s.encode('latin-1') if isinstance(s, str) else bytes(s)      # noqa: E731
  for d, w in zip(descs, windows):
    reads, haplotypes = [as_bytes(r) for r in w['reads']], [as_bytes(h) for h in w['haplotypes']]
    d.first_read, d.n_reads = len(raw), len(reads)
    raw += reads
    d.first_haplotype, d.n_haplotypes = len(raw), len(haplotypes)
    raw += haplotypes
    d.reference = len(raw)
    raw.append(as_bytes(w['reference']))
    d.ref_prefix_len, d.ref_suffix_len = w.get('ref_prefix_len', 0), w.get('ref_suffix_len', 0)
    d.ref_start = w.get('ref_start', 0)
  off = np.zeros(len(raw) + 1, np.int64)
  np.cumsum([len(b) for b in raw], out=off[1:])
  table = b''.join(raw)
  opt = _lib.DvAlignerOptions()
  for name, value in (options or {}).items():
    setattr(opt, name, value)
  handle = C.c_void_p()
  args = [len(raw), table, off.ctypes.data, len(windows), descs, C.byref(opt), C.byref(handle)]
  if stream is not None:
    args.append(stream or None)
  _lib.check(entry(*args))
  try:
    view = _lib.DvAlignedWindowsView()
    _lib.check(_lib.lib().dv_aligned_windows_arrays(handle, C.byref(view)))
    take = lambda ptr, n, ctype, dtype: (np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(n,)).copy()   # noqa: E731
                                         if n else np.zeros(0, dtype))
    return dict(window_read_off=take(view.window_read_off, view.n_windows + 1, C.c_int32, np.int32),
                status=take(view.status, view.n_reads, C.c_int32, np.int32),
                position=take(view.position, view.n_reads, C.c_int64, np.int64),
                cigar_off=take(view.cigar_off, view.n_reads + 1, C.c_uint32, np.uint32),
                cigar=take(view.cigar, view.n_words, C.c_uint32, np.uint32))
  finally:
    _lib.lib().dv_aligned_windows_free(handle)


def align_windows_batch(windows: Sequence[dict], options: Optional[dict] = None):
  """FastPassAligner.AlignReads for every window of a batch, host code (dv_align_windows_batch).  A window is
  dict(reads=[...], haplotypes=[...], reference=str, ref_prefix_len=0, ref_suffix_len=0, ref_start=0); reads are
  upper-cased by the call.  `options`: fields of dv_aligner_options (0 or absent keeps the class default).
  -> dict(window_read_off int32[w + 1], status int32[r], position int64[r], cigar_off uint32[r + 1], cigar uint32[...])
  over the reads of all windows in window order."""
  return _align_windows(_lib.lib().dv_align_windows_batch, windows, options, None)


def align_windows_batch_device(windows: Sequence[dict], options: Optional[dict] = None, stream: int = 0,
                               with_stats: bool = False):
  """`align_windows_batch` end to end on the device: the fast pass, the sweeps with their trace-back and the finish
  kernels of csrc/realign_finish.hip; identical arrays.  A window with a pair outside the sweep or trace-back
  kernel's limits is finished by the host code inside the call.  There is no CPU fallback: without a GPU this raises
  DV_ERR_NO_DEVICE.  with_stats: -> (arrays, _lib.DvRealignFinishStats)."""
  res = _align_windows(_lib.lib().dv_align_windows_batch_device, windows, options, stream)
  if not with_stats:
    return res
  stats = _lib.DvRealignFinishStats()
  _lib.check(_lib.lib().dv_realign_finish_last_stats(C.byref(stats)))
  return res, stats


def realign_reads_to_haplotype(haplotype: str, reads: Sequence, contig: str, ref_start: int, ref_end: int,
                               ref_reader, aln_config: Optional[dict] = None) -> List[Optional[T.Read]]:
  """RealignReadsToHaplotype (alt_aligned_pileup_lib.cc:278-313).

  Returns one entry per input read: the read with its new alignment, the unchanged read
  (the merged CIGAR came out empty), or None where the reference returns an empty Read."""
  cfg = dict(aln_config or {})
  cfg['read_size'] = (len(reads[0].aligned_sequence)
                      if reads and len(reads[0].aligned_sequence) > 15 else 200)
  ext_start = max(0, ref_start - K_REF_ALIGN_MARGIN)
  ext_end = min(ref_reader.n_bases(contig), ref_end + K_REF_ALIGN_MARGIN)
  prefix = ref_reader.get_bases(contig, ext_start, ref_start) if ext_start < ref_start else ''
  suffix = ref_reader.get_bases(contig, ref_end, ext_end) if ref_end < ext_end else ''
  target = prefix + haplotype + suffix
  aligner = FastPassAligner(force_alignment=True, ref_prefix_len=ref_start - ext_start,
                            ref_suffix_len=ext_end - ref_end, **cfg)
  aligner.set_reference(target, ext_start)
  aligner.set_haplotypes([target])
  return aligner.realign_reads(reads)
