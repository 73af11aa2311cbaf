/*
 * dvhip.h -- C ABI of libdvhip.so, the MI355X (gfx950) implementation of
 * DeepVariant's make_examples -> call_variants hot path.
 *
 * This is the drop-in boundary.  Every entry point is `extern "C"`, takes plain
 * pointers and sizes (no torch / protobuf / STL types), and replaces one piece
 * of the reference's native hot path; the reference interface each one
 * replaces is cited as file:line relative to google/deepvariant v1.10.0.
 * INTEGRATION.md shows the pybind/ctypes stub a reference maintainer would add.
 *
 * Conventions
 *   - Return value: DV_OK (0) or a negative dv_status; dv_last_error() gives a
 *     thread-local message.  Conditions the reference CHECK-fails on
 *     (LOG(FATAL)) are reported as errors, never silently patched.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  All
 *     device work is enqueued on it; calls that write HOST memory synchronise
 *     the stream before returning, calls that only touch device memory do not.
 *   - Pointers inside dv_batch are host or device pointers according to
 *     dv_batch.memory.  Device pointers must be 4-byte aligned.
 *   - There is NO CPU fallback: without a HIP device every compute entry
 *     point returns DV_ERR_NO_DEVICE.
 */
#ifndef DVHIP_H_
#define DVHIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DV_ABI_VERSION 8
#define DV_MAX_CHANNELS 16
#define DV_READ_AUX_STRIDE 8

typedef enum dv_status {
  DV_OK = 0,
  DV_ERR_INVALID_ARGUMENT = -1,
  DV_ERR_UNSUPPORTED = -2, /* e.g. a channel the device encoder does not draw */
  DV_ERR_NO_DEVICE = -3,
  DV_ERR_HIP = -4,
  DV_ERR_OUT_OF_MEMORY = -5,
  DV_ERR_BAD_INPUT = -6, /* what the reference would CHECK-fail / LOG(FATAL) on */
} dv_status;

typedef enum dv_memory { DV_MEM_HOST = 0, DV_MEM_DEVICE = 1 } dv_memory;

/* DeepVariantChannelEnum values, deepvariant/protos/deepvariant.proto:1287-1342. */
enum {
  DV_CH_READ_BASE = 1,
  DV_CH_BASE_QUALITY = 2,
  DV_CH_MAPPING_QUALITY = 3,
  DV_CH_STRAND = 4,
  DV_CH_READ_SUPPORTS_VARIANT = 5,
  DV_CH_BASE_DIFFERS_FROM_REF = 6,
  DV_CH_HAPLOTYPE_TAG = 7,
  DV_CH_ALLELE_FREQUENCY = 8,          /* pixel supplied in list_aux */
  DV_CH_READ_MAPPING_PERCENT = 11,     /* pixel supplied in read_aux[0] */
  DV_CH_AVG_BASE_QUALITY = 12,         /* read_aux[1] */
  DV_CH_IDENTITY = 13,                 /* read_aux[2] */
  DV_CH_GAP_COMPRESSED_IDENTITY = 14,  /* read_aux[3] */
  DV_CH_GC_CONTENT = 15,               /* read: read_aux[4]; reference row: ref_aux2 */
  DV_CH_IS_HOMOPOLYMER = 16,           /* per base: base_aux0; reference row: ref_aux0 */
  DV_CH_HOMOPOLYMER_WEIGHTED = 17,     /* per base: base_aux1; reference row: ref_aux1 */
  DV_CH_BLANK = 18,
  DV_CH_INSERT_SIZE = 19,
  DV_CH_MEAN_COVERAGE = 22,
  DV_CH_BASE_METHYLATION = 23,
  DV_CH_BASE_6MA = 24,
  DV_CH_READ_SUPPORTS_VARIANT_FUZZY = 25, /* pixel supplied in list_aux */
  DV_CH_SUPPLEMENTARY_ALIGNMENT = 26,
  DV_CH_ALLELE_SAMPLE_PROBABILITY = 27, /* pixel supplied in list_aux */
  /* Ultima flow-space channels (channels/homopolymer_{insertion,deletion}_quality_channel.cc,
   * channels/inter_homopolymer_insertion_quality_channel.cc): per-base pixels the host computes from the tp / t0
   * aux tags (dv_flow_channel_pixels) and passes in the base_aux planes, see dv_batch */
  DV_CH_HOMOPOLYMER_INSERTION_QUALITY = 28,
  DV_CH_HOMOPOLYMER_DELETION_QUALITY = 29,
  DV_CH_INTER_HOMOPOLYMER_INSERTION_QUALITY = 30,
};

/* CIGAR op codes = nucleus CigarUnit::Operation
 * (third_party/nucleus/protos/cigar.proto:38-82); cigar[] = (len << 4) | op. */
enum {
  DV_CIGAR_ALIGNMENT_MATCH = 1,
  DV_CIGAR_INSERT = 2,
  DV_CIGAR_DELETE = 3,
  DV_CIGAR_SKIP = 4,
  DV_CIGAR_CLIP_SOFT = 5,
  DV_CIGAR_CLIP_HARD = 6,
  DV_CIGAR_PAD = 7,
  DV_CIGAR_SEQUENCE_MATCH = 8,
  DV_CIGAR_SEQUENCE_MISMATCH = 9,
};

/* read_flags bits */
enum {
  DV_READ_REVERSE = 1,       /* alignment.position.reverse_strand */
  DV_READ_SUPPLEMENTARY = 2, /* supplementary_alignment */
  DV_READ_HAS_5MC = 4,       /* base_modifications has k5mC */
  DV_READ_HAS_6MA = 8,       /* base_modifications has k6mA */
};

#define DV_HP_NONE INT32_MIN /* read has no (single, integer) HP tag */

/* POD image of the PileupImageOptions fields the encoder reads
 * (deepvariant/protos/deepvariant.proto:500-638; defaults in
 * deepvariant/pileup_image.py:36-74).  `channels` is what
 * PileupImageEncoderNative::AllChannelsEnum("") returns
 * (deepvariant/pileup_image_native.cc:125-151). */
typedef struct dv_encoder_options {
  int32_t width;  /* = ref_bases.size(); the odd-width CHECK of pileup_image_native.cc:114 is the host mirror's */
  int32_t height;
  int32_t reference_band_height;
  int32_t n_channels;
  int32_t channels[DV_MAX_CHANNELS];
  int32_t base_color_offset_a_and_g;
  int32_t base_color_offset_t_and_c;
  int32_t base_color_stride;
  float allele_supporting_read_alpha;
  float allele_unsupporting_read_alpha;
  float other_allele_supporting_read_alpha;
  float reference_matching_read_alpha;
  float reference_mismatching_read_alpha;
  int32_t indel_anchoring_base_char;
  int32_t reference_base_quality;
  int32_t positive_strand_color;
  int32_t negative_strand_color;
  int32_t base_quality_cap;
  int32_t mapping_quality_cap;
  int32_t min_base_quality;    /* read_requirements.min_base_quality */
  int32_t min_mapping_quality; /* read_requirements.min_mapping_quality */
  uint32_t random_seed;
  int32_t sort_by_haplotypes;
  int32_t hp_tag_for_assembly_polishing;
  int32_t sort_by_alt_allele_support;
  float min_non_zero_allele_frequency;
} dv_encoder_options;

/*
 * A packed batch of pileup "items".  One item = one call of
 * PileupImageEncoderNative::BuildPileupForOneSample
 * (deepvariant/pileup_image_native.cc:297-447) followed by the kNone branch of
 * FillPileupArray (deepvariant/pileup_image_native.h:214-275): one candidate x
 * one alt-allele combination x one sample.  Multi-sample stacking and the
 * `rows` / `single_row` alt-aligned layouts are several items whose
 * item_out_off place them one below the other in the same example.
 *
 * Reads are a structure of arrays shared by all items of the batch (a read
 * overlaps many candidates).  Strings never reach the device: the host
 * resolves read names into
 *   read_name_rank  dense rank of (fragment_name, read_number) under the
 *                   reference's tie-break order (pileup_image_native.cc:97-101)
 *   list_code       ReadSupportsVariantChannel::ReadSupportsAlt: 0/1/2
 *                   (deepvariant/channels/read_supports_variant_channel.cc:75-104)
 *   list_group      allele-support sort group (pileup_image_native.cc:346-393)
 * per (item, read).
 */
typedef struct dv_batch {
  int32_t memory; /* dv_memory: where every pointer below lives */

  /* ---- reads (n_reads) ---- */
  int32_t n_reads;
  const int32_t* read_pos;        /* alignment.position.position */
  const int32_t* read_sort_pos;   /* original (pre-trim) position; NULL = read_pos */
  const uint32_t* read_seq_off;   /* [n_reads+1] into bases / quals / mods */
  const uint32_t* read_cigar_off; /* [n_reads+1] into cigar */
  const uint8_t* read_mapq;       /* alignment.mapping_quality (<= 255) */
  const uint8_t* read_flags;      /* DV_READ_* */
  const int32_t* read_frag_len;   /* fragment_length */
  const int32_t* read_hp;         /* HP tag value or DV_HP_NONE */
  const uint32_t* read_name_rank;
  const uint8_t* read_aux;        /* [n_reads][DV_READ_AUX_STRIDE] or NULL */
  const uint8_t* bases;           /* aligned_sequence, ASCII */
  const uint8_t* quals;           /* aligned_quality, raw phred */
  const uint8_t* mod_5mc;         /* parallel to bases, or NULL */
  const uint8_t* mod_6ma;
  const uint32_t* cigar;          /* (operation_length << 4) | operation */
  uint32_t n_bases;               /* = read_seq_off[n_reads] */
  uint32_t n_cigar;               /* = read_cigar_off[n_reads] */

  /* ---- items (n_items) ---- */
  int32_t n_items;
  const int32_t* item_variant_start; /* dv_call.variant.start */
  const int32_t* item_image_start;   /* image_start_pos (may be negative) */
  const uint32_t* item_ref_idx;      /* row of ref_windows */
  const uint32_t* item_list_off;     /* [n_items+1] into list_* */
  const uint16_t* item_height;       /* sample pileup_height (rows of this item) */
  const uint64_t* item_out_off;      /* byte offset of the item's row 0 in `out` */
  const uint32_t* item_blank_mask;   /* bit c = channel index c blanked for reads; NULL = 0 */
  const float* item_mean_coverage;   /* NULL = 0.0 */
  const uint8_t* ref_windows;        /* [n_ref_windows][width] ASCII, N-padded */
  uint32_t n_ref_windows;

  /* ---- per (item, read) lists, in InMemoryReader::Query order
   * (deepvariant/make_examples_native.cc:802-810); the encoder applies
   * DownsampleReadIndices itself ---- */
  const uint32_t* list_read;  /* read index */
  const uint8_t* list_code;   /* 0 / 1 / 2 */
  const uint8_t* list_group;  /* NULL = 0 */
  const uint8_t* list_aux;    /* NULL; host-computed pixel for DV_CH_ALLELE_* */
  uint32_t n_list;            /* = item_list_off[n_items] */
  uint32_t max_list_len;      /* upper bound on any item's list length */

  /* ---- sequence-context channels (channels/{is_homopolymer,homopolymer_weighted,
   * gc_content}_channel.cc): host-computed PIXELS, all optional (NULL unless the channel
   * list asks for them) ---- */
  const uint8_t* base_aux0; /* parallel to bases: is_homopolymer pixel of every read base */
  const uint8_t* base_aux1; /* parallel to bases: homopolymer_weighted pixel */
  const uint8_t* ref_aux0;  /* [n_ref_windows][width]: is_homopolymer pixel of the window */
  const uint8_t* ref_aux1;  /* [n_ref_windows][width]: homopolymer_weighted pixel */
  const uint8_t* ref_aux2;  /* [n_ref_windows][width]: gc_content pixel of the window, repeated */
  /* ABI v6.  A third per-base plane, and the rule that assigns planes: is_homopolymer always reads base_aux0 and
   * homopolymer_weighted base_aux1; each flow-space channel (DV_CH_HOMOPOLYMER_INSERTION_QUALITY, _DELETION_QUALITY,
   * DV_CH_INTER_HOMOPOLYMER_INSERTION_QUALITY), in the order of the channel list, takes the first plane of
   * base_aux2, base_aux1, base_aux0 that no other channel of the list reads (dv_base_aux_plane answers for a given
   * list).  Their reference-row pixel is 0.  More than three per-base channels in one list: DV_ERR_UNSUPPORTED. */
  const uint8_t* base_aux2;
  /* ABI v7.  Optional hints (0 = unknown) that size the encoder's per-item LDS tables: an upper bound on the
   * CIGAR operations of any read and on any item_height.  With them the row pipeline keeps up to 64 operations
   * per kept read in LDS (8 without: reads with more take the row-at-a-time path -- every ONT read).  A host
   * batch is measured by dv_encode_batch itself; a DV_MEM_DEVICE batch relies on the hints, and a hint that
   * is too small is a caller error (items are clamped to it, never read out of bounds). */
  uint32_t max_cigar_ops;
  uint32_t max_item_height;
} dv_batch;

typedef struct dv_encoder dv_encoder;
typedef struct dv_model dv_model;

/* Which base_aux plane (0, 1, 2) the channel at index `channel_index` of `channels[n_channels]` (DV_CH_* values)
 * reads; DV_BASE_AUX_NONE if it reads none; a dv_status (< 0) otherwise: DV_ERR_UNSUPPORTED if the list needs more
 * planes than there are. */
#define DV_BASE_AUX_NONE 3
int dv_base_aux_plane(const int32_t* channels, int32_t n_channels, int32_t channel_index);

/* SampleOptions.use_non_uniform_downsampling (deepvariant/pileup_image_native.cc:242-294,326-341;
 * deepvariant/sampling_util.h:57-155): the reads of one pile-up that survive when every allele keeps at least
 * `min_per_partition` of its supporters.  part_off[n_parts + 1] / part_idx: for every allele of
 * DeepVariantCall.allele_support, in the order the map yields them, the indices (into the pile-up's read list,
 * 0 .. n_reads - 1) of the reads it lists, and as the LAST element the reads no allele lists (GetReadIndicesAllelePartition
 * finds reads by their "fragment_name/read_number" key: of several reads with one key only the last takes part -- the
 * others appear in no element and are never drawn).  A read listed twice belongs to the first element that lists it.
 * out[<= n_reads] receives the sample in ascending order, *n_out its size -- or -1 where the reference's
 * sampler fails (the thresholds alone exceed max_reads) and BuildPileupForOneSample falls back to the uniform
 * shuffle: the caller then passes the whole list to dv_encode_batch as usual.  With a sample in hand the caller passes
 * only those reads (the list is then no longer than max_reads and the device draws them all, in that order).
 * Draws: absl::Uniform over std::mt19937_64(random_seed), restated (csrc/sampling.cpp: parity UNPINNED for the bit
 * stream alone).  forced_draws (tests; NULL otherwise) replaces the draws, one per Uniform(0, index) call. */
int dv_downsample_with_partition_mins(int32_t n_reads, const int32_t* part_off, const int32_t* part_idx,
                                      int32_t n_parts, int32_t max_reads, int32_t min_per_partition,
                                      uint32_t random_seed, const uint64_t* forced_draws, int64_t n_forced,
                                      int32_t* out, int32_t* n_out);

/* Per-base pixels of a flow-space channel for every read of a table, to be passed as the base_aux plane the channel
 * reads (channels/homopolymer_indel_quality_channel.cc:68-183, channels/inter_homopolymer_insertion_quality_channel.cc:
 * 76-125, channels/channel_utils.cc:41-44).  `tags` is parallel to bases:
 *   DV_CH_HOMOPOLYMER_INSERTION_QUALITY / _DELETION_QUALITY   the tp tag's values (0 where a read has none or fewer)
 *   DV_CH_INTER_HOMOPOLYMER_INSERTION_QUALITY                 the t0 tag's characters - 33 (0 where a read has none)
 * Host arithmetic as in the reference (double pow, float sum, float log10); no device work. */
int dv_flow_channel_pixels(int channel, const uint8_t* bases, const uint8_t* quals, const int8_t* tags,
                           const uint32_t* read_seq_off, int32_t n_reads, uint8_t* out);

const char* dv_last_error(void);
int dv_abi_version(void);
/* Number of visible HIP devices (0 without a GPU). */
int dv_device_count(void);

/* ---------------------------------------------------------------- encoder */

/* PileupImageEncoderNative::PileupImageEncoderNative
 * (deepvariant/pileup_image_native.cc:111-123).  Builds the pixel LUTs with the
 * reference's fp32 arithmetic on the host and uploads them. */
int dv_encoder_create(const dv_encoder_options* options, int device,
                      dv_encoder** out);
void dv_encoder_destroy(dv_encoder* enc);

/* BuildPileupForOneSample + FillPileupArray for every item of the batch
 * (deepvariant/pileup_image_native.cc:297-447,
 *  deepvariant/pileup_channel_lib.cc:91-261, deepvariant/channels/ *.cc,
 *  deepvariant/pileup_image_native.h:214-275), one workgroup per item.
 *   out           uint8, item i row r at out + item_out_off[i] + r*width*out_channels,
 *                 pixels HWC with `out_channels` >= n_channels bytes each
 *                 (extra trailing channels are zero-filled; at most 64)
 *                 A workgroup stages four rows of width*out_channels bytes in LDS next to its read tables: a
 *                 shape whose request exceeds 64 KiB is DV_ERR_INVALID_ARGUMENT (dv_last_error names the width
 *                 and out_channels) before anything is copied or launched.
 *   out_rows     int32[n_items] read rows kept per item, may be NULL
 *   out_memory    dv_memory of out / out_rows */
int dv_encode_batch(dv_encoder* enc, const dv_batch* batch, int out_channels,
                    uint8_t* out, int32_t* out_rows, int out_memory,
                    void* stream);

/* The checks dv_encode_batch applies to a HOST batch before staging it: what the
 * reference LOG(FATAL)s / CHECKs on (unknown CIGAR op, pileup_channel_lib.cc:252; a CIGAR
 * that consumes more bases than aligned_sequence holds) and every index range the kernel
 * trusts.  A caller that uploads its own DV_MEM_DEVICE batch (device batches are not
 * readable from the host) runs this on the host image first.  Host only, no device work. */
int dv_validate_batch(const dv_batch* batch, int32_t reference_band_height);

/* DownsampleReadIndices (deepvariant/pileup_image_native.cc:153-165): iota,
 * std::shuffle'd with std::mt19937_64(seed) iff n > max_reads.  Host only. */
int dv_downsample_indices(int n, int max_reads, uint32_t seed, int32_t* out);

/* InMemoryReader::Query + nucleus::ReadOverlapsRegion for every item
 * (deepvariant/make_examples_native.cc:802-810,
 *  third_party/nucleus/util/utils.cc:172-240) over packed HOST reads:
 * item i gets the reads r (ascending index = caller order) with
 *   query_end[i] > read_pos[r] && query_start[i] < read_end(r).
 * Two-pass: call with list_read == NULL to get counts in list_off[n_items+1],
 * then again with a buffer of list_off[n_items] entries. */
int dv_query_reads(int32_t n_reads, const int32_t* read_pos,
                   const uint32_t* read_cigar_off, const uint32_t* cigar,
                   int32_t n_items, const int64_t* query_start,
                   const int64_t* query_end, uint32_t* list_off,
                   uint32_t* list_read);

/* ---- BAM -> packed read table (host only) --------------
 * Replaces SamReader::Query + ConvertToPb + InMemoryReader construction
 * (third_party/nucleus/io/sam_reader.cc:734-840, deepvariant/make_examples_core.py:
 * region_reads_norealign) for the fields the encoder consumes.  dv_read_requirements
 * mirrors nucleus.genomics.v1.ReadRequirements
 * (third_party/nucleus/protos/reads.proto:421-445; sam_reader.cc:217-247,
 *  third_party/nucleus/util/utils.cc:261-266); make_examples' defaults are all zero
 * except min_mapping_quality (deepvariant/make_examples_options.py:954-990). */
typedef struct dv_read_requirements {
  int32_t keep_duplicates;
  int32_t keep_failed_vendor_quality_checks;
  int32_t keep_secondary_alignments;
  int32_t keep_supplementary_alignments;
  int32_t keep_improperly_placed;
  int32_t min_mapping_quality;
  /* SamReaderOptions.use_original_base_quality_scores (third_party/nucleus/io/sam_reader.cc:722-740):
   * qualities come from the OQ:Z aux tag (char - 33) instead of QUAL.  nucleus leaves
   * aligned_quality EMPTY for a read without the tag -- which the encoder cannot draw -- so
   * here such a read is an error (DV_ERR_BAD_INPUT). */
  int32_t use_original_base_quality_scores;
  /* ABI v6: per-base planes from aux tags, what make_examples asks SamReader to parse when the channel list needs
   * them (deepvariant/make_examples_core.py:288-373 resolve_sam_aux_fields).
   * parse_base_modifications: MM / ML / MN -> 5mC and 6mA planes = Read.base_modifications
   * (third_party/nucleus/io/sam_reader.cc:521-719 ParseBaseModifications, :855-862); dv_read_table_fill_batch then
   * sets dv_batch::mod_5mc / mod_6ma, and read_flags carry DV_READ_HAS_5MC / DV_READ_HAS_6MA per read.
   * parse_flow_tags: the Ultima tp (B array) and t0 (Z) tags -> dv_read_table_aux_planes' tp / t0 planes, the
   * `tags` input of dv_flow_channel_pixels. */
  int32_t parse_base_modifications;
  int32_t parse_flow_tags;
} dv_read_requirements;

typedef struct dv_read_table dv_read_table; /* owns host arrays in dv_batch's read layout */

/* Reads `path` (BGZF BAM).  With `<path>.bai` present and a contig given, only the BGZF
 * members the index points at are read; otherwise the whole file is inflated on
 * `n_threads` threads.  Keeps the mapped reads of `contig` (NULL = all) that overlap
 * [start, end) (nucleus::ReadOverlapsRegion) and satisfy `req` (NULL = keep nothing
 * optional, mapq >= 0), in file order. */
int dv_bam_read_region(const char* path, const char* contig, int64_t start, int64_t end,
                       const dv_read_requirements* req, int n_threads, dv_read_table** out);
/* ---- CRAM 3.0 -> the same packed read table (host only) ------------------------
 * Replaces the CRAM side of SamReader (third_party/nucleus/io/sam_reader.cc:560-640: hts_open +
 * hts_set_opt(CRAM_OPT_REFERENCE) for SamReaderOptions.ref_path / --use_ref_for_cram, :1022-1035
 * the query iterator, :734-840 ConvertToPb).  `fetch` supplies the bases of the FASTA the file
 * was written against: it is asked for [start, end) of `contig` (0-based, half open), writes up to
 * end - start bases into `out` (fewer at a contig's end: *n_out), returns 0 on success; it may be
 * entered from a worker thread of the call, one thread at a time.  NULL = decode from the slices'
 * embedded references only (--nouse_ref_for_cram); a slice that needs the external reference is
 * then DV_ERR_BAD_INPUT, as is a FASTA whose MD5 differs from the slice header's.  With
 * `<path>.crai` present and a contig given, only the containers the index lists are decoded
 * (without one the container headers are walked); slices decode on `n_threads` threads.  Same
 * rows, in the same order, dv_bam_read_region returns for the BAM of the same alignments. */
typedef int (*dv_ref_fetch_fn)(void* ctx, const char* contig, int64_t start, int64_t end,
                               char* out, int64_t* n_out);
int dv_cram_read_region(const char* path, const char* contig, int64_t start, int64_t end,
                        const dv_read_requirements* req, dv_ref_fetch_fn fetch, void* fetch_ctx,
                        int n_threads, dv_read_table** out);
/* The optional per-base planes of a table, parallel to its bases (NULL where the requirements did not ask for them):
 * 5mC / 6mA modification probabilities; tp values (0 where a read has no tag or a shorter one); t0 characters - 33;
 * flow_present[read]: bit 0 = the read has a tp tag, bit 1 = a t0 tag.  Any output pointer may be NULL. */
int dv_read_table_aux_planes(const dv_read_table* table, const uint8_t** mod_5mc, const uint8_t** mod_6ma,
                             const int8_t** tp, const uint8_t** t0, const uint8_t** flow_present);
/* The SAM header text of a CRAM (its first container): `needed` = its length; up to
 * `capacity` bytes are copied to `text` (may be NULL). */
int dv_cram_header(const char* path, char* text, uint64_t capacity, uint64_t* needed);
/* Points the read-table fields of `b` (n_reads, read_*, bases, quals, cigar, n_bases,
 * n_cigar; memory = DV_MEM_HOST) at the table's arrays; item / list fields are left
 * alone.  The table must outlive the batch. */
int dv_read_table_fill_batch(const dv_read_table* t, dv_batch* b);
/* fragment_name (NUL-terminated) and read_number of read i: the key
 * "<fragment_name>/<read_number>" DeepVariantCall.allele_support refers to. */
const char* dv_read_table_name(const dv_read_table* t, int32_t i, int32_t* read_number);
/* All names at once: NUL-terminated strings in `blob` (blob_bytes long), name i at
 * blob + offsets[i], read_numbers[i] in {0, 1}. */
int dv_read_table_names(const dv_read_table* t, const char** blob, const uint32_t** offsets,
                        const uint8_t** read_numbers, uint64_t* blob_bytes);
/* exclusive reference end of every read (alignment start + reference span) */
const int64_t* dv_read_table_ends(const dv_read_table* t);
void dv_read_table_free(dv_read_table* t);

/* ---- candidates + region reads -> item / list arrays (host only) -------------
 * Replaces the per-candidate decisions of ExamplesGenerator::
 * CreateAndWriteExamplesForCandidate that precede the pixels
 * (deepvariant/make_examples_native.cc:632-736): InMemoryReader::Query per
 * candidate (:645-648,802-810), one item per alt-allele combination (:191-267),
 * and per (item, read) the ReadSupportsAlt code
 * (deepvariant/channels/read_supports_variant_channel.cc:54-116) and allele group
 * (deepvariant/pileup_image_native.cc:346-393) from DeepVariantCall.allele_support.
 * Single sample; multi-sample stacking stays with the host mirror. */
typedef struct dv_pack_reads {
  int32_t n_reads;
  const int32_t* read_pos;     /* alignment start */
  const int64_t* read_end;     /* exclusive reference end (dv_read_table_ends) */
  const char* names;           /* NUL-terminated fragment names, concatenated */
  const uint32_t* name_off;    /* [n_reads] offset of each name in `names` */
  const uint8_t* read_number;  /* [n_reads] 0 / 1: the key is "<name>/<read_number>" */
} dv_pack_reads;

typedef struct dv_pack_options {
  int32_t width;                   /* pic_options.width: image_start = variant.start - (width-1)/2 */
  int32_t read_overlap_buffer_bp;  /* pic_options.read_overlap_buffer_bp (5) */
  int32_t pileup_height;           /* sample_options.pileup_height */
  int32_t n_threads;               /* host threads over the candidates; 0 / 1 = the calling thread only */
  uint64_t example_bytes;          /* bytes of one example: item k is written at k * example_bytes */
} dv_pack_options;

typedef struct dv_pack_candidate {
  int64_t start, end;       /* variant.start, variant.end */
  int32_t n_alts;           /* variant.alternate_bases_size (<= 32) */
  int32_t ref_idx;          /* index of its reference window in the batch's ref_windows; < 0 = none
                               (contig edge): the candidate is skipped like the reference does */
  uint32_t first_combo, n_combos;      /* slice of combo_masks: bit i = alternate_bases[i] is in the combination */
  uint32_t first_support, n_support;   /* slice of the support arrays */
} dv_pack_candidate;

typedef struct dv_packed_region dv_packed_region; /* owns the item / list arrays */

/* support_keys: NUL-terminated "<fragment_name>/<read_number>" strings (allele_support
 * read_names), support_key_off[j] the offset of entry j, support_alt[j] the index in
 * alternate_bases of the allele that lists it. */
int dv_pack_region(const dv_pack_reads* reads, const dv_pack_options* opt, int32_t n_candidates,
                   const dv_pack_candidate* cands, const uint32_t* combo_masks,
                   const char* support_keys, const uint32_t* support_key_off,
                   const uint8_t* support_alt, dv_packed_region** out);
/* Points the item / list fields of `b` (n_items, n_list, max_list_len, item_*, list_read,
 * list_code, list_group iff use_groups) at the packed arrays; read-table, reference-window
 * and per-item option fields (blank mask, mean coverage) are the caller's. */
int dv_packed_region_fill_batch(const dv_packed_region* p, int use_groups, dv_batch* b);
/* Which (candidate, combination mask) each item is; returns the item count. */
int dv_packed_region_items(const dv_packed_region* p, const int32_t** item_candidate,
                           const uint32_t** item_combo);
void dv_packed_region_free(dv_packed_region* p);

/* ---- the same for a batch of regions, on the device, read support by ROW -------------
 * dv_pack_region's arrays for several regions at once, computed by three kernels (csrc/pack_regions.hip: count,
 * scan, emit) and LEFT in device memory for dv_encode_batch.  No string is involved: a read is known by an integer
 * key, and a candidate's support lists name keys.  dv_pack_region stays the checker: for one region the arrays are
 * equal, array for array.
 *   rows       the regions' read tables, concatenated.  read_key[r] is equal for two rows of one region iff their
 *              "<fragment_name>/<read_number>" keys are equal (keys are compared within a region only); NULL =
 *              every row is its own key, and a support entry then names the row in the concatenated table.
 *   regions    region k owns rows [read_first, read_first + n_reads) and candidates [cand_first, cand_first +
 *              n_cands); the candidate slices follow each other in region order and cover cands[n_candidates].
 *   cands      as dv_pack_region's; ref_idx indexes the reference windows of the whole batch, first_support /
 *              n_support slice support_key / support_alt (an entry whose key matches no picked read is ignored).
 * Items are numbered across the batch, in region order then candidate order; list_read is the row in the
 * concatenated table; item_candidate is the index into cands. */
typedef struct dv_pack_rows {
  int32_t n_reads;
  const int32_t* read_pos;   /* alignment start */
  const int64_t* read_end;   /* exclusive reference end */
  const int32_t* read_key;   /* [n_reads] or NULL */
} dv_pack_rows;

typedef struct dv_pack_region_slice {
  int32_t read_first, n_reads;
  int32_t cand_first, n_cands;
} dv_pack_region_slice;

typedef struct dv_pack_regions_options {
  int32_t width;                   /* as dv_pack_options */
  int32_t read_overlap_buffer_bp;
  int32_t pileup_height;
  int32_t n_candidates;            /* entries of cands */
  uint32_t n_combo_masks;          /* entries of combo_masks */
  uint32_t n_support;              /* entries of support_key / support_alt */
  uint64_t example_bytes;          /* item k is written at k * example_bytes */
  float mean_coverage;             /* item_mean_coverage of every item */
} dv_pack_regions_options;

typedef struct dv_packed_regions dv_packed_regions; /* owns the item / list arrays, in device memory */

/* One upload, pack_count_kernel and pack_scan_kernel, one small download and one synchronisation (the totals and
 * max_list_len), one allocation, pack_emit_kernel -- all on `stream` (NULL = a non-blocking stream the library owns,
 * which the call then also waits for).  With a caller's stream the arrays are ready in stream order: hand the same
 * stream to dv_encode_batch.  Placement is a pure function of the input (no atomics): two calls give identical bytes.
 * DV_ERR_INVALID_ARGUMENT before any device work, *out NULL: null pointers, negative counts, slices outside their
 * arrays, and for a candidate with a reference window n_alts outside [0, 32] or a support_alt >= n_alts;
 * width < 3, pileup_height <= 0.  No candidate with a reference window and a combination: DV_OK, an empty handle,
 * no device needed.  Otherwise no device is DV_ERR_NO_DEVICE (dv_pack_region is the host code).  More than
 * 2^32 - 1 list entries or 2^31 - 1 items: DV_ERR_BAD_INPUT, decided from the counts before anything is emitted. */
int dv_pack_regions_device(int32_t n_regions, const dv_pack_region_slice* regions, const dv_pack_rows* rows,
                           const dv_pack_regions_options* opt, const dv_pack_candidate* cands,
                           const uint32_t* combo_masks, const int32_t* support_key, const uint8_t* support_alt,
                           void* stream, dv_packed_regions** out);
/* Points the item / list fields of `b` -- whose memory must be DV_MEM_DEVICE -- at the arrays (list_group iff
 * use_groups), sets n_items, n_list, max_list_len, item_blank_mask = NULL (0) and item_mean_coverage (the options'
 * value for every item); read-table and reference-window fields and the size hints are the caller's. */
int dv_packed_regions_fill_batch(const dv_packed_regions* p, int use_groups, dv_batch* b);
typedef struct dv_packed_regions_view {   /* host copies; valid until the handle is freed */
  int32_t n_items;
  uint32_t n_list, max_list_len;
  const int32_t* item_variant_start;
  const int32_t* item_image_start;
  const uint32_t* item_ref_idx;
  const uint32_t* item_list_off;      /* [n_items + 1] */
  const uint16_t* item_height;
  const uint64_t* item_out_off;
  const float* item_mean_coverage;
  const int32_t* item_candidate;
  const uint32_t* item_combo;
  const uint32_t* list_read;
  const uint8_t* list_code;
  const uint8_t* list_group;
} dv_packed_regions_view;
/* Waits for the emit kernel and copies the arrays to the host (once; later calls return the same copies). */
int dv_packed_regions_download(dv_packed_regions* p, dv_packed_regions_view* out);
/* Which (candidate, combination mask) each item is, in host memory; returns the item count. */
int dv_packed_regions_items(const dv_packed_regions* p, const int32_t** item_candidate, const uint32_t** item_combo);
void dv_packed_regions_free(dv_packed_regions* p);
typedef struct dv_pack_device_stats {
  int64_t regions;
  int64_t candidates;
  int64_t items;
  int64_t list_entries;
  int64_t regions_unsorted;   /* regions whose read_pos does not ascend: their candidates scan the whole slice */
  int64_t launches;
} dv_pack_device_stats;
/* What the calling thread's last dv_pack_regions_device did. */
int dv_pack_regions_device_last_stats(dv_pack_device_stats* out);

/* ---- the same handle for items whose read list is GIVEN: a row range of a table ----------
 * A trimmed or alt-aligned region draws window-cut COPIES of its reads: every candidate owns a row range of the
 * trimmed table and every (candidate, alt) a row range of the alt-aligned one, so there is no position query -- only
 * the per-read rule of dv_pack_regions_device remains.  A `draw` is one encoder item: its list is the rows
 * row_first .. row_first + n_rows - 1 of the concatenated table, in that order, and its record (reference window,
 * starts, height, out_off, mean coverage) is the caller's -- alt images go to scratch rows behind the examples, so
 * out_off is not item * example_bytes.
 *   rows_key   int32 per row of the concatenated table: two rows carry equal values iff they are copies of one read
 *              key of ONE region (the caller keeps the ids of different regions apart); NULL = every row is its own
 *              key, and a support entry then names a row.
 *   cands      dv_pack_candidate with only n_alts, first_support and n_support read (its slice of support_key /
 *              support_alt); start, end, ref_idx, first_combo and n_combos are ignored -- the draw carries them.
 * Per row r of a draw of candidate c: first_alt is the smallest support_alt among c's entries with r's key and group
 * the largest; with no such entry first_alt = 255 and group = n_alts; list_code = 0 for 255, 1 if bit first_alt of
 * combo_mask is set, else 2; list_group = group.  An entry whose key matches no row is ignored.
 * Every size is known before the launch (item_list_off is the prefix sum of n_rows, max_list_len the largest n_rows):
 * one upload, one allocation at the exact size, one launch (pack_draws_kernel, one wave per draw) and no
 * synchronisation -- with a caller's stream the call returns without waiting and the arrays are ready in stream order;
 * with stream NULL it waits for the library's own stream, as dv_pack_regions_device does.  Two calls give identical
 * bytes.  The handle is dv_pack_regions_device's: dv_packed_regions_fill_batch, _download, _items and _free work on
 * it unchanged (item_candidate / item_combo are the draws' cand / combo_mask).
 * DV_ERR_INVALID_ARGUMENT before any device work, *out NULL: null pointers with non-zero counts or negative counts; a
 * draw whose row range leaves [0, n_rows), whose cand is outside [0, n_cands) or whose height is 0; a candidate's
 * support slice outside the arrays, n_alts outside [0, 32] or a support_alt >= n_alts; a combo_mask bit at or above
 * n_alts.  More than 2^31 - 1 draws or 2^32 - 1 list entries: DV_ERR_BAD_INPUT.  No draw: DV_OK, an empty handle, no
 * device needed.  Otherwise no device is DV_ERR_NO_DEVICE. */
typedef struct dv_pack_draw {
  int32_t cand;             /* index into cands */
  uint32_t combo_mask;      /* bit i = alternate_bases[i] is in the combination */
  int32_t row_first, n_rows;
  uint32_t ref_idx;         /* item_ref_idx */
  int32_t variant_start;    /* item_variant_start */
  int32_t image_start;      /* item_image_start */
  uint16_t height;          /* item_height (> 0) */
  uint64_t out_off;         /* item_out_off */
  float mean_coverage;      /* item_mean_coverage */
} dv_pack_draw;

int dv_pack_draws_device(const int32_t* rows_key, int32_t n_rows, const dv_pack_draw* draws, int64_t n_draws,
                         const dv_pack_candidate* cands, int32_t n_cands, const int32_t* support_key,
                         const uint8_t* support_alt, uint32_t n_support, void* stream, dv_packed_regions** out);
typedef struct dv_pack_draws_stats {
  int64_t draws;
  int64_t candidates;
  int64_t list_entries;
  int64_t launches;
} dv_pack_draws_stats;
/* What the calling thread's last dv_pack_draws_device did. */
int dv_pack_draws_device_last_stats(dv_pack_draws_stats* out);

/* ---- read realigner (host only) ----------------------------------------------
 * Replaces deepvariant/realigner/fast_pass_aligner.{h,cc} (class FastPassAligner) and the
 * local aligner it links (libssw v1.2.5 through deepvariant/realigner/ssw.{h,cc}); used by
 * RealignReadsToHaplotype for alt-aligned pileups (deepvariant/alt_aligned_pileup_lib.cc:
 * 278-313).  Options follow AlignerOptions (deepvariant/protos/realigner.proto:178-228):
 * 0 keeps the class default. */
typedef struct dv_aligner dv_aligner;

typedef struct dv_aligner_options {
  int32_t match, mismatch, gap_open, gap_extend;          /* defaults 4, 6, 8, 1 */
  int32_t kmer_size, read_size, max_num_of_mismatches;    /* defaults 32, 100, 2 */
  double realignment_similarity_threshold;                /* default 0.85 */
  int32_t force_alignment;   /* never return the original alignment (alt-aligned pileups) */
  int32_t normalize_reads;   /* --normalize_reads: keep alignments that could shift left */
  int32_t ref_prefix_len, ref_suffix_len;   /* reference padding around the haplotype */
} dv_aligner_options;

typedef struct dv_realigned_read {
  int32_t status;      /* 0 = original alignment kept, 1 = new alignment, 2 = read dropped
                          (force_alignment and no alignment found: the reference returns an empty Read) */
  int32_t n_cigar;
  int64_t position;    /* new alignment start (reference coordinates), status 1 only */
  uint32_t cigar_off;  /* first word of its CIGAR in the array dv_aligner_align_reads returns */
  uint32_t reserved;
} dv_realigned_read;

typedef struct dv_read_alignment {   /* ReadAlignment (fast_pass_aligner.h:104-128) */
  int32_t position;    /* offset in the haplotype; -1 = kNotAligned */
  int32_t score;
  char cigar[120];     /* text, as the reference keeps it ("15=", "3S3=2I13=") */
} dv_read_alignment;

typedef struct dv_local_alignment {  /* StripedSmithWaterman::Alignment, the fields used */
  int32_t score, ref_begin, ref_end, query_begin, query_end, mismatches;
  char cigar[512];
} dv_local_alignment;

int dv_aligner_create(const dv_aligner_options* options, dv_aligner** out);   /* set_options */
void dv_aligner_destroy(dv_aligner* a);
int dv_aligner_set_reference(dv_aligner* a, const char* reference, int64_t ref_start); /* set_reference + set_ref_start */
int dv_aligner_set_haplotypes(dv_aligner* a, int32_t n, const char* const* haplotypes);
int dv_aligner_set_reads(dv_aligner* a, int32_t n, const char* const* reads);
/* FastPassAligner::AlignReads.  `cigar` receives (length << 4 | op) words -- nucleus op
 * codes, dv_batch's CIGAR encoding -- owned by the aligner until its next call. */
int dv_aligner_align_reads(dv_aligner* a, int32_t n, const char* const* sequences,
                           dv_realigned_read* out, const uint32_t** cigar);
/* Individual stages, for tests that follow fast_pass_aligner_test.cc. */
enum {
  DV_ALIGNER_BUILD_INDEX = 0,        /* BuildIndex */
  DV_ALIGNER_INIT_LOCAL_ALIGNER = 1, /* InitSswLib */
  DV_ALIGNER_ALIGN_HAPLOTYPES = 2,   /* AlignHaplotypesToReference */
  DV_ALIGNER_POSITION_MAPS = 3,      /* CalculatePositionMaps */
  DV_ALIGNER_LOCAL_ALIGN_READS = 4,  /* SswAlignReadsToHaplotypes(arg = score threshold) */
  DV_ALIGNER_SCORE_THRESHOLD = 5,    /* CalculateSswAlignmentScoreThreshold */
  DV_ALIGNER_ALIGN_IN_PHASES = 6     /* test hook: arg != 0 makes dv_aligner_align_reads run as the device route
                                        does -- prepare, ONE batch of pairs through the host aligner, finish;
                                        arg == 2 also splits the prepare step as DV_REALIGN_DEVICE_FASTPASS does --
                                        reads, dv_fast_pass_batch's host code with its arrays installed, pairs --
                                        and never builds the k-mer index */
};
int dv_aligner_stage(dv_aligner* a, int32_t stage, int32_t arg);
int dv_aligner_fast_align(dv_aligner* a, const char* haplotype, int32_t* haplotype_score,
                          dv_read_alignment* out /* [n reads] */);   /* FastAlignReadsToHaplotype */
int dv_aligner_haplotype_info(const dv_aligner* a, int32_t k, int32_t* haplotype_index,
                              int32_t* haplotype_score, int64_t* ref_pos, int32_t* is_reference,
                              char* cigar, int32_t cigar_cap);
int dv_aligner_read_alignment(const dv_aligner* a, int32_t k, int32_t read, dv_read_alignment* out);
/* CalculateReadToRefAlignment; the merged CIGAR as text with M / I / D / S. */
int dv_aligner_merge_alignment(const dv_aligner* a, int32_t read, int32_t position,
                               const char* read_cigar, const char* haplotype_cigar, char* out, int32_t cap);
int dv_aligner_is_normalized(const dv_aligner* a, const char* cigar, int32_t ref_offset,
                             const char* read);                          /* 1 / 0 */
int dv_aligner_score_threshold(const dv_aligner* a);
/* Occurrences of a k-mer in the read index (count returned); "" returns the number of k-mers. */
int dv_aligner_kmer_occurrences(const dv_aligner* a, const char* kmer, int32_t cap, int32_t* reads,
                                int32_t* offsets);
int dv_positions_map(const char* cigar, int32_t haplotype_size, int32_t* out);        /* SetPositionsMap */
int dv_merge_cigar_op(char* cigar, int32_t cap, char op, int32_t length, int32_t read_len); /* MergeCigarOp */
/* One local alignment (Aligner::SetReferenceSequence + Align). */
int dv_local_align(const char* reference, const char* query, int32_t match, int32_t mismatch,
                   int32_t gap_open, int32_t gap_extend, dv_local_alignment* out);
/* The same for n queries against one reference, 16 alignments per SIMD batch (the path the
 * realigner uses for haplotypes -> reference and reads -> haplotypes); identical results.
 * out[k].score = -1 where dv_local_align would fail (empty query). */
int dv_local_align_many(const char* reference, int32_t n, const char* const* queries, int32_t match,
                        int32_t mismatch, int32_t gap_open, int32_t gap_extend, dv_local_alignment* out);

/* The same alignments with the two Smith-Waterman sweeps on the device (csrc/local_align.hip): one upload,
 * one kernel launch and one download for the whole list, on `stream` (a hipStream_t; NULL = a
 * non-blocking stream the library owns); CIGARs are built on the host from the corner points, or from
 * the device's M/I/D runs (below).
 * Sequences are ASCII: sequence s is bases[seq_off[s], seq_off[s + 1]); pair k aligns query
 * pair_query[k] to reference pair_ref[k], so a sequence that many pairs share is uploaded once.
 * out[k] is what dv_local_align(reference, query, ...) returns; out[k].score = -1 where it would fail
 * (an empty sequence).  A pair outside the kernel's limits below is aligned by the host code
 * inside the same call.  Argument errors (null pointers, descending offsets, an index out of
 * range, negative counts, match outside [1, 127] or a penalty outside [0, 127] -- the host
 * class keeps its score matrix in int8_t) are DV_ERR_INVALID_ARGUMENT before any device work;
 * n_pairs = 0 is DV_OK without a device; no device is DV_ERR_NO_DEVICE. */
#define DV_LOCAL_ALIGN_DEVICE_MAX_QUERY 2048        /* bases of a query the kernel holds in registers */
#define DV_LOCAL_ALIGN_DEVICE_MAX_REFERENCE 65534   /* bases of a reference */
typedef struct dv_realign_device_stats {
  int64_t pairs;          /* alignments asked for */
  int64_t pairs_on_host;  /* of them outside the kernel's limits: aligned by the host code */
  int64_t cells;          /* sum of |reference| * |query| over the forward passes on the device */
  int64_t launches;       /* kernel launches */
} dv_realign_device_stats;
int dv_local_align_pairs_device(int32_t n_seqs, const char* bases, const int64_t* seq_off, int32_t n_pairs,
                                const int32_t* pair_ref, const int32_t* pair_query, int32_t match,
                                int32_t mismatch, int32_t gap_open, int32_t gap_extend,
                                dv_local_alignment* out, void* stream);
/* What the calling thread's last dv_local_align_pairs_device did (for tests and tools). */
int dv_local_align_device_last_stats(dv_realign_device_stats* out);

/* The banded trace-back on the device.  For a pair the kernel has swept and that holds an alignment
 * (score > 0 and the reverse pass reached it) the same launch also runs LocalAligner::banded_cigar
 * between the corner points -- the band |ref_len - q_len| + 1, doubling until the score is reached, and
 * the walk back from the bottom-right cell -- and returns the M/I/D runs; the host is left with the text
 * form (soft clips, '=' / 'X', mismatches).  One diagonal of the band per lane, so a pair goes back to
 * the host's banded_cigar, inside the same call and with the same result, when its band would pass
 * DV_LOCAL_ALIGN_DEVICE_MAX_BAND, when its runs do not fit DV_LOCAL_ALIGN_DEVICE_MAX_RUNS, when the
 * call's direction-byte scratch (256 MiB, about 64 bytes per query base) is used up, or when banded_cigar
 * itself would fail.  DV_REALIGN_DEVICE_TRACEBACK=0 / 1 in the environment, read at each call, turns it
 * off / on for both device entry points; unset it is off (DESIGN.md section 12 has the measurement). */
#define DV_LOCAL_ALIGN_DEVICE_MAX_BAND 31   /* 2 * band + 1 diagonals in the 64 lanes of a wave */
#define DV_LOCAL_ALIGN_DEVICE_MAX_RUNS 64   /* M/I/D runs of one alignment */
typedef struct dv_realign_traceback_stats {
  int64_t traced_on_device;  /* swept pairs holding an alignment whose runs came from the device */
  int64_t traced_on_host;    /* ... and those that LocalAligner's host code traced back */
  int64_t band_cells;        /* sum over the former of q_len * (2 * band + 1), final band: cells of its last DP */
  int64_t widest_band;       /* the largest final band among the former */
} dv_realign_traceback_stats;
/* What the calling thread's last dv_local_align_pairs_device or dv_realign_regions_device did. */
int dv_local_align_device_last_traceback_stats(dv_realign_traceback_stats* out);
/* Host only, no device: the band banded_cigar ends with and the number of M/I/D runs of the CIGAR that
 * dv_local_align(reference, query, ...) returns, which decide whether the device traces the pair back;
 * 0 / 0 where there is no CIGAR (nothing aligns, or dv_local_align fails). */
int dv_local_align_band(const char* reference, const char* query, int32_t match, int32_t mismatch,
                        int32_t gap_open, int32_t gap_extend, int32_t* band, int32_t* runs);

/* ---- the fast pass over many windows in one call -----------------------------------
 * FastPassAligner::FastAlignReadsToHaplotype (fast_pass_aligner.cc:207-286) for every (window, haplotype)
 * of a batch, without the k-mer index and without its order dependence.  For a haplotype H of n bytes, a read
 * R of L bytes (upper-cased by the call), k = kmer_size, M = max_num_of_mismatches:
 *   - a read with L <= k or L > n takes no part;
 *   - a seed is (i, off) with H[i..i+k) == R[off..off+k) byte for byte ('N' equals only 'N'); it names the
 *     start s = max(0, i - off), which takes part when s + L <= n; the discovery key of (R, s) is its
 *     lexicographically smallest seed;
 *   - mm(R, s) counts the positions p with H[s+p] != R[p] where neither byte is 'N'; (R, s) is accepted when
 *     it has a seed and mm <= M; its score is (L - mm) * match - mm * mismatch;
 *   - a read's alignment is its accepted start with the largest score > 0, the smallest discovery key on
 *     ties; none: position -1, score 0;
 *   - every accepted (R, s) covers haplotype positions [key.i, s + L); a haplotype whose bytes differ from
 *     the window's reference is discarded (score 0, no alignments) when a position i <= n - k with
 *     ref_prefix_len <= i < n - ref_suffix_len stays uncovered although H[i..i+k) occurs in some read longer
 *     than k (the host looks at a position's coverage only after its k-mer was found in the index);
 *   - the haplotype's score is the sum of its reads' scores.
 * Sequences are raw bytes: sequence s is bytes[seq_off[s], seq_off[s + 1]).  Haplotypes are taken as given.
 * Haplotype h of the call is the h-th of all windows' haplotypes in window order, and its reads' rows are
 * [sum of n_reads over the haplotypes before it, + its window's n_reads).  read_position is -1 where the read is
 * not aligned.  options: as dv_aligner_create (0 keeps the class default; only match, mismatch, kmer_size and
 * max_num_of_mismatches are read).  Argument errors (null pointers, negative counts or lengths, descending
 * offsets, a range or index outside the table, options the class refuses) are DV_ERR_INVALID_ARGUMENT
 * before any device work. */
typedef struct dv_fast_pass_window {
  int32_t first_read, n_reads;             /* its reads: sequences [first_read, first_read + n_reads) */
  int32_t first_haplotype, n_haplotypes;   /* its haplotypes: sequences [first_haplotype, ...) */
  int32_t reference;                       /* the sequence holding the window's reference, or -1: no haplotype is it */
  int32_t ref_prefix_len, ref_suffix_len;  /* reference padding around the haplotypes */
  int32_t reserved;
} dv_fast_pass_window;
/* Host code (FastPassAligner itself, k-mer index included). */
int dv_fast_pass_batch(int32_t n_seqs, const char* bytes, const int64_t* seq_off, int32_t n_windows,
                       const dv_fast_pass_window* windows, const dv_aligner_options* options, void* stream,
                       int32_t* haplotype_score, int32_t* haplotype_discarded, int32_t* read_position,
                       int32_t* read_score);
/* The same on the device (csrc/fast_pass.hip): one upload, ONE kernel launch over every (window, haplotype),
 * one download and one synchronisation on `stream` (NULL = a non-blocking stream the library owns); identical
 * arrays.  A haplotype longer than DV_FAST_PASS_DEVICE_MAX_HAPLOTYPE (it lives in LDS beside its coverage
 * marks; reads are never longer than their haplotype) or scoring values past DV_FAST_PASS_DEVICE_MAX_SCORING
 * are not an error: the host code runs that haplotype inside the same call.  No haplotypes is DV_OK without a
 * device; no device is DV_ERR_NO_DEVICE (there is no CPU fallback). */
#define DV_FAST_PASS_DEVICE_MAX_HAPLOTYPE 8192
#define DV_FAST_PASS_DEVICE_MAX_SCORING 32767
int dv_fast_pass_batch_device(int32_t n_seqs, const char* bytes, const int64_t* seq_off, int32_t n_windows,
                              const dv_fast_pass_window* windows, const dv_aligner_options* options, void* stream,
                              int32_t* haplotype_score, int32_t* haplotype_discarded, int32_t* read_position,
                              int32_t* read_score);
typedef struct dv_fast_pass_stats {
  int64_t haplotypes;          /* (window, haplotype) items asked for */
  int64_t haplotypes_on_host;  /* of them outside the kernel's limits: run by the host code */
  int64_t pairs;               /* (haplotype, read) pairs of the items on the device */
  int64_t cells;               /* diagonals x read length over those pairs: byte comparisons at most */
  int64_t launches;            /* kernel launches */
} dv_fast_pass_stats;
/* What the calling thread's last dv_fast_pass_batch_device or dv_realign_regions_device did with the fast
 * pass (all zero when the latter ran it on the host: DV_REALIGN_DEVICE_FASTPASS unset). */
int dv_fast_pass_device_last_stats(dv_fast_pass_stats* out);

/* ---- window trimming of reads on a packed table -------------------------------------
 * TrimReads (deepvariant/alt_aligned_pileup_lib.cc:231-248) for many pileup windows over one region's read
 * table: per window, the rows with q1 > read_pos && q0 < read_end, in row order (InMemoryReader::Query), each
 * cut to [r0, r1) (TrimRead / TrimCigar, :91-216) and kept when its trimmed CIGAR spans >= min_overlap
 * reference bases and holds at least one read base.  The closed form is written out in csrc/trim_reads.hip;
 * the Python restatement is alt_aligned_pileup_lib.trim_cigar / trim_read / trim_reads.
 * `reads` is a DV_MEM_HOST dv_batch of which read_pos, read_seq_off, read_cigar_off and cigar are read;
 * read_end (alignment ends, [n_reads]) is not part of dv_batch and comes beside it.  The table may be unsorted.
 * A pair with r1 <= max(r0, read_pos) (the reference's CHECK_GT) or whose trimmed CIGAR needs more bases than the
 * read's sequence has is DV_ERR_BAD_INPUT for the whole call; dv_last_error names the smallest such (window, row).
 * Null pointers, negative counts, a table not in host memory, descending offsets, ends or window bounds outside
 * int32: DV_ERR_INVALID_ARGUMENT before any device work.  On any error *out is NULL and nothing stays allocated. */
typedef struct dv_trim_window {
  int64_t q0, q1;        /* the read query: variant start / end -/+ read_overlap_buffer_bp */
  int64_t r0, r1;        /* the pileup window (CalculateAlignmentRegion) */
  int32_t min_overlap;   /* kDefaultMinimumReadOverlap (15), or the image width for window-spanning reads only */
  int32_t reserved;
} dv_trim_window;
typedef struct dv_trimmed_reads dv_trimmed_reads;   /* owns the host arrays of one call's result */
typedef struct dv_trimmed_reads_view {              /* views into the result; valid until dv_trimmed_reads_free */
  int32_t n_windows;
  int32_t n_rows;                  /* kept (window, read) pairs: the same read once per window that keeps it */
  int64_t n_words;
  const int32_t* window_row_off;   /* [n_windows + 1]: window w's rows are [off[w], off[w + 1]) */
  const int32_t* src_row;          /* [n_rows] the row of `reads` */
  const int32_t* pos;              /* r0 where the window cut the read's start, else read_pos */
  const int32_t* end;              /* pos + the reference span of the trimmed CIGAR */
  const int32_t* read_trim;        /* the kept bases are [read_trim, read_trim + new_len) of the read's */
  const int32_t* new_len;
  const uint32_t* cigar_off;       /* [n_rows + 1] into cigar */
  const uint32_t* cigar;           /* [n_words] dv_batch's encoding; a CIGAR the window ends inside an operation
                                      of closes with that operation at its remaining length, which may be 0 */
} dv_trimmed_reads_view;
/* Host code (csrc/trim_reads.hip, TrimCigar operation by operation); for tests and tools. */
int dv_trim_reads_batch(const dv_batch* reads, const int64_t* read_end, int32_t n_windows,
                        const dv_trim_window* windows, dv_trimmed_reads** out);
/* The same on the device: one wave per (window, read) pair; one upload, three launches (count, scan, emit), one
 * download and one synchronisation on `stream` (NULL = a non-blocking stream the library owns); identical arrays.
 * CIGAR length is unbounded.  No pair at all is DV_OK without a device; no device is DV_ERR_NO_DEVICE (there is
 * no CPU fallback). */
int dv_trim_reads_batch_device(const dv_batch* reads, const int64_t* read_end, int32_t n_windows,
                               const dv_trim_window* windows, dv_trimmed_reads** out, void* stream);
int dv_trimmed_reads_arrays(const dv_trimmed_reads* t, dv_trimmed_reads_view* out);
void dv_trimmed_reads_free(dv_trimmed_reads* t);
typedef struct dv_trim_stats {
  int64_t pairs_tested;    /* (window, read) pairs that passed the overlap test: one wave each */
  int64_t pairs_kept;
  int64_t words_read;      /* CIGAR operations of the tested pairs (the kernel stops at the window's end) */
  int64_t words_written;
  int64_t launches;
} dv_trim_stats;
/* What the calling thread's last dv_trim_reads_batch_device did. */
int dv_trim_device_last_stats(dv_trim_stats* out);

/* ---- alt-aligned realignment on a packed table --------------------------------------
 * RealignReadsToHaplotype (deepvariant/alt_aligned_pileup_lib.cc:278-313) for many (candidate, sample, alt allele)
 * items over one table of trimmed reads.  Per item the reference builds a FastPassAligner whose one haplotype IS its
 * reference (the target), with force_alignment and no reference padding: the haplotype is never discarded, its CIGAR
 * to the reference is one match run, the score threshold decides nothing.  For pair (item t, read R of L bytes --
 * upper-cased by the call --, target T of n bytes, taken as given):
 *   - choice: the fast pass' position p (dv_fast_pass_batch's contract, T both haplotype and reference) gives
 *     read-to-haplotype "<L>=" at p; otherwise dv_local_align(T, R) with score > 0 gives p = (uint16_t)ref_begin and
 *     its CIGAR, soft clips included; otherwise status 2;
 *   - merge: CalculateReadToRefAlignment against "<n>=": p >= n is status 0; a leading soft clip is taken as it is;
 *     every other operation of the read is cut where the n - p haplotype bases end (an insertion takes none of them)
 *     and goes through MergeCigarOp -- lengths capped so that the read-consuming ones sum to L at most, an insertion
 *     beside a deletion cancelling base by base into matches planted in front of the indel --; past the haplotype's
 *     end the remaining operations are merged whole, a cut soft clip's tail too; a cut operation of any other kind
 *     left over clears the CIGAR (status 0);
 *   - normalisation: IsAlignmentNormalized of the merged CIGAR against T at offset p and the read's bytes, unless
 *     options->normalize_reads; not normalised is status 0;
 *   - result: status 1, position = ref_start + p, the merged CIGAR.  An empty CIGAR is status 0.
 * `reads` is a DV_MEM_HOST dv_batch of which only bases and read_seq_off are read (alt_aligned_pileup_lib.trim_table's
 * output).  Targets are raw bytes: target s is target_bytes[target_off[s], target_off[s + 1]).  Items may share rows
 * (two alts of one candidate name the same range).  options: as dv_aligner_create (0 keeps the class default), with
 * read_size taken from each item; force_alignment must be 1 and ref_prefix_len / ref_suffix_len 0.
 * Null pointers, negative counts, descending offsets, a row range or target index outside its table, a negative
 * ref_start, a table not in host memory, options outside the above or that the class refuses:
 * DV_ERR_INVALID_ARGUMENT before any device work.  On any error *out is NULL and nothing stays allocated. */
typedef struct dv_alt_align_item {
  int32_t first_row, n_rows;   /* its reads: rows [first_row, first_row + n_rows) of `reads` */
  int32_t target;              /* index into the target table */
  int32_t read_size;           /* AlignerOptions.read_size: the first read's length if it exceeds 15, else 200 */
  int64_t ref_start;           /* reference coordinate of target[0] */
  int64_t reserved;
} dv_alt_align_item;
typedef struct dv_alt_aligned dv_alt_aligned;   /* owns the host arrays of one call's result */
typedef struct dv_alt_aligned_view {            /* views into the result; valid until dv_alt_aligned_free */
  int32_t n_items;
  int32_t n_pairs;                 /* (item, row) pairs: item order, then row order */
  int64_t n_words;
  const int32_t* item_pair_off;    /* [n_items + 1]: item t's pairs are [off[t], off[t + 1]) */
  const int32_t* status;           /* [n_pairs] 0 / 1 / 2 as dv_realigned_read */
  const int64_t* position;         /* [n_pairs] status 1 only, else 0 */
  const uint32_t* cigar_off;       /* [n_pairs + 1] into cigar; words only for status 1 */
  const uint32_t* cigar;           /* [n_words] dv_batch's encoding */
} dv_alt_aligned_view;
/* Host code (csrc/alt_align.hip): FastPassAligner::AlignReads item by item, what dv_aligner_* does for Read objects.
 * The checker of the device route, and the route of the items outside its limits. */
int dv_alt_align_batch(const dv_batch* reads, int32_t n_items, const dv_alt_align_item* items, int32_t n_targets,
                       const char* target_bytes, const int64_t* target_off, const dv_aligner_options* options,
                       dv_alt_aligned** out);
/* The same on the device: the fast pass of every item in one launch (csrc/fast_pass.hip), the Smith-Waterman sweeps
 * of every pair it did not place in one launch (csrc/local_align.hip; trace-back as DV_REALIGN_DEVICE_TRACEBACK says),
 * and three launches (count, scan, emit; one lane per pair) that merge, check and compact every pair's CIGAR; three
 * round trips on `stream` (NULL = a non-blocking stream the library owns); identical arrays.  An item whose target is
 * longer than DV_FAST_PASS_DEVICE_MAX_HAPLOTYPE (or reaches 65,535 bytes: positions are uint16_t) is not an error:
 * the host code runs it inside the call; so is a pair outside DV_LOCAL_ALIGN_DEVICE_MAX_*.  No pair at all is DV_OK
 * without a device; no device is DV_ERR_NO_DEVICE (there is no CPU fallback). */
int dv_alt_align_batch_device(const dv_batch* reads, int32_t n_items, const dv_alt_align_item* items,
                              int32_t n_targets, const char* target_bytes, const int64_t* target_off,
                              const dv_aligner_options* options, dv_alt_aligned** out, void* stream);
int dv_alt_aligned_arrays(const dv_alt_aligned* a, dv_alt_aligned_view* out);
void dv_alt_aligned_free(dv_alt_aligned* a);
typedef struct dv_alt_align_stats {
  int64_t items;              /* items asked for */
  int64_t items_on_host;      /* of them outside the fast pass' limits: run whole by the host code */
  int64_t pairs;              /* (item, row) pairs */
  int64_t pairs_fast;         /* placed by the fast pass */
  int64_t pairs_swept;        /* sent through Smith-Waterman (pairs = pairs_fast + pairs_swept) */
  int64_t pairs_swept_on_host;   /* of them outside the sweep kernel's limits, or of an item on the host */
  int64_t pairs_traced_on_host;  /* swept on the device, holding an alignment, traced back by the host code */
  int64_t status0, status1, status2;
  int64_t words_written;
  int64_t launches;           /* kernel launches: fast pass + sweeps + the three finish kernels */
} dv_alt_align_stats;
/* What the calling thread's last dv_alt_align_batch_device did. */
int dv_alt_align_device_last_stats(dv_alt_align_stats* out);

/* ---- the window aligner over many windows in one call -------------------------------
 * FastPassAligner::AlignReads (deepvariant/realigner/fast_pass_aligner.cc:131-177) for a batch of windows, each with
 * its own reads, haplotypes and reference: what dv_aligner_create / set_reference / set_haplotypes /
 * dv_aligner_align_reads do per window, in one call and with the result as arrays.
 * Sequences are raw bytes: sequence s is bytes[seq_off[s], seq_off[s + 1]); reads are upper-cased by the call,
 * haplotypes and the reference are taken as given.  options: as dv_aligner_create (0 keeps the class default;
 * read_size and force_alignment are the call's, normalize_reads too; ref_prefix_len / ref_suffix_len come from each
 * window).  Per read of every window, in window order then read order: status (0 / 1 / 2 as dv_realigned_read),
 * position and the merged CIGAR (status 1 only).
 * Null pointers, negative counts or lengths, descending offsets, a range or index outside the table, a window
 * without a reference, a negative ref_start, options the class refuses or scoring values past 127:
 * DV_ERR_INVALID_ARGUMENT before any device work.  On any error *out is NULL and nothing stays allocated. */
typedef struct dv_align_window {
  int32_t first_read, n_reads;             /* its reads: sequences [first_read, first_read + n_reads) */
  int32_t first_haplotype, n_haplotypes;   /* its haplotypes: sequences [first_haplotype, ...) */
  int32_t reference;                       /* the sequence holding the window's reference (required) */
  int32_t ref_prefix_len, ref_suffix_len;  /* reference padding around the haplotypes */
  int32_t reserved;
  int64_t ref_start;                       /* reference coordinate of reference[0] */
} dv_align_window;
typedef struct dv_aligned_windows dv_aligned_windows;   /* owns the host arrays of one call's result */
typedef struct dv_aligned_windows_view {                /* views into the result; valid until dv_aligned_windows_free */
  int32_t n_windows;
  int32_t n_reads;                 /* of all windows */
  int64_t n_words;
  const int32_t* window_read_off;  /* [n_windows + 1]: window w's reads are [off[w], off[w + 1]) */
  const int32_t* status;           /* [n_reads] 0 / 1 / 2 as dv_realigned_read */
  const int64_t* position;         /* [n_reads] status 1 only, else 0 */
  const uint32_t* cigar_off;       /* [n_reads + 1] into cigar; words only for status 1 */
  const uint32_t* cigar;           /* [n_words] dv_batch's encoding */
} dv_aligned_windows_view;
/* Host code (csrc/realign_finish.hip): FastPassAligner::align_reads window by window.  The checker of the device form. */
int dv_align_windows_batch(int32_t n_seqs, const char* bytes, const int64_t* seq_off, int32_t n_windows,
                           const dv_align_window* windows, const dv_aligner_options* options,
                           dv_aligned_windows** out);
/* The same end to end on the device: the fast pass of every (window, haplotype) in one launch (csrc/fast_pass.hip),
 * one download, the pairs collected on the host, every pair's sweeps and trace-back in one launch
 * (csrc/local_align.hip) whose result stays on the device -- of a pair only its corners, traced flag, run count and band
 * come down --, then the finish kernels of csrc/realign_finish.hip, one lane per haplotype and then per (window, read):
 * haplotype states, best haplotype + merge counted, scan, merge written; one staged upload, one download, one
 * synchronisation on `stream` (NULL = a non-blocking stream the library owns); identical arrays.  A window is finished
 * on the device only if every one of its pairs was swept there and every pair that holds an alignment was traced back
 * there (DV_LOCAL_ALIGN_DEVICE_MAX_*, the trace-back's scratch budget); any other window is finished by the host code
 * inside the call, with the host's trace-back for its pairs, and counted.  No read at all is DV_OK without a device;
 * no device is DV_ERR_NO_DEVICE (there is no CPU fallback).  The device holds room for 64 CIGAR words per read of the
 * call; a call with more runs its launches a second time with the exact room.  DV_REALIGN_FINISH_ROOM=1..64 in the
 * environment, read at each call, lowers that room (for tests of the second run; results are identical). */
int dv_align_windows_batch_device(int32_t n_seqs, const char* bytes, const int64_t* seq_off, int32_t n_windows,
                                  const dv_align_window* windows, const dv_aligner_options* options,
                                  dv_aligned_windows** out, void* stream);
int dv_aligned_windows_arrays(const dv_aligned_windows* a, dv_aligned_windows_view* out);
void dv_aligned_windows_free(dv_aligned_windows* a);
typedef struct dv_realign_finish_stats {
  int64_t windows;          /* windows with reads that reached the finish step */
  int64_t windows_on_host;  /* of them handed back: finished by FastPassAligner::finish_alignments */
  int64_t reads;            /* reads finished on the device */
  int64_t cigar_words;      /* words of their merged CIGARs */
  int64_t launches;         /* finish kernel launches */
  int64_t bytes_down;       /* downloaded by the sweep call (8 words per pair) and by the finish step */
} dv_realign_finish_stats;
/* What the calling thread's last dv_align_windows_batch_device or dv_realign_regions_device did with the finish step
 * (all zero when the latter did not use it: DV_REALIGN_DEVICE_FINISH unset). */
int dv_realign_finish_last_stats(dv_realign_finish_stats* out);
/* Test hook, host only: the order FastPassAligner's std::sort by haplotype_score gives n haplotype alignments with
 * these scores, computed over (score, index) records (order_records, what the device route uploads) and over real
 * HaplotypeAlignment objects (order_objects); both [n]. */
int dv_realign_finish_sorted_order(int32_t n, const int32_t* scores, int32_t* order_records, int32_t* order_objects);

/* ---- local assembly for the window realigner ------------------------------------
 * Replaces deepvariant/realigner/debruijn_graph.{h,cc} (DeBruijnGraph::Build,
 * CandidateHaplotypes, GraphViz; python binding deepvariant/realigner/python/
 * debruijn_graph_pybind.cc).  Options are DeBruijnGraphOptions (deepvariant/protos/
 * realigner.proto).  Reads come as the region's packed read table (dv_batch's bases / quals /
 * read_seq_off / read_mapq arrays) plus the indices of the reads that overlap the window, in
 * the order the reference would add them. */
typedef struct dv_debruijn_graph dv_debruijn_graph;

typedef struct dv_debruijn_options {
  int32_t min_k, max_k, step_k;
  int32_t min_mapq, min_base_quality, min_edge_weight, max_num_paths;
  int32_t disable_graph_pruning;
} dv_debruijn_options;

/* *out = NULL (and DV_OK) when no k gives an acyclic graph: debruijn_graph.build() -> None. */
int dv_debruijn_build(const char* ref, int64_t ref_len, const uint8_t* bases, const uint8_t* quals, int64_t n_bases,
                      const uint32_t* read_seq_off, const uint8_t* read_mapq, int32_t n_table_reads,
                      const int32_t* reads, int32_t n_reads, const dv_debruijn_options* options,
                      dv_debruijn_graph** out);
void dv_debruijn_destroy(dv_debruijn_graph* g);
int dv_debruijn_kmer_size(const dv_debruijn_graph* g);                                 /* kmer_size */
/* candidate_haplotypes(): sorted; strings owned by the graph until its next call. */
int dv_debruijn_haplotypes(dv_debruijn_graph* g, int32_t* n, const char* const** haplotypes);
int dv_debruijn_graphviz(dv_debruijn_graph* g, const char** text);                     /* graphviz */

/* The graph of the winning k BEFORE pruning, as integers ("compact form"), for many windows in one call.  An
 * occurrence is (seq, pos): seq 0 is the window's reference, seq 1 + j the j-th read of its list (a read below
 * min_mapq keeps its number and never occurs), pos the offset of the k-mer's first byte.  Vertices and edges are
 * in insertion order, which is ascending first occurrence (the constructor walks the reference, then the reads in
 * order, each left to right), so the form is canonical; an edge's occurrence is that of its `from` k-mer in the
 * walk that created the edge.  Sequence s is bases / quals [seq_off[s], seq_off[s + 1]); mapq has one entry per
 * sequence (a reference's is not read).  k[w] = 0: dv_debruijn_build returns NULL for the window.  k_tries[w] is
 * the number of k values of the schedule visited, the reference-repeat test's included. */
typedef struct dv_debruijn_window {
  int32_t reference;               /* the sequence holding the window's reference */
  int32_t first_read, n_reads;     /* its reads: sequences [first_read, first_read + n_reads) */
  int32_t reserved;
} dv_debruijn_window;
typedef struct dv_debruijn_compact {   /* views into the result; valid until dv_debruijn_compact_free */
  const int32_t* k;                /* [n_windows] */
  const int32_t* k_tries;          /* [n_windows] */
  const int64_t* vertex_off;       /* [n_windows + 1] into the vertex arrays */
  const int32_t* vertex_seq;
  const int32_t* vertex_pos;
  const int64_t* edge_off;         /* [n_windows + 1] into the edge arrays */
  const int32_t* edge_from;        /* vertex numbers within the window */
  const int32_t* edge_to;
  const int32_t* edge_weight;
  const int32_t* edge_is_ref;
  const int32_t* edge_seq;
  const int32_t* edge_pos;
} dv_debruijn_compact;
typedef struct dv_debruijn_compact_result dv_debruijn_compact_result;
/* Host code (DeBruijnGraph's own constructor and cycle test). */
int dv_debruijn_compact_batch(int32_t n_seqs, const char* bases, const uint8_t* quals, const int64_t* seq_off,
                              const uint8_t* mapq, int32_t n_windows, const dv_debruijn_window* windows,
                              const dv_debruijn_options* options, dv_debruijn_compact_result** out,
                              dv_debruijn_compact* arrays);
void dv_debruijn_compact_free(dv_debruijn_compact_result* r);
/* The same on the device (csrc/debruijn.hip has the contract without the maps): one upload, ONE kernel launch with
 * a workgroup per window -- the choice of k and the cycle test included --, one download and one synchronisation on
 * `stream` (NULL = a non-blocking stream the library owns); identical arrays.  A window whose reference plus reads
 * pass DV_DEBRUIJN_DEVICE_MAX_BASES, or whose graph at some k passes DV_DEBRUIJN_DEVICE_MAX_VERTICES /
 * DV_DEBRUIJN_DEVICE_MAX_EDGES (found at run time), is not an error: the host code builds it inside the same call.
 * No device is DV_ERR_NO_DEVICE (there is no CPU fallback). */
#define DV_DEBRUIJN_DEVICE_MAX_VERTICES 8192
#define DV_DEBRUIJN_DEVICE_MAX_EDGES 8192
#define DV_DEBRUIJN_DEVICE_MAX_BASES 131072
int dv_debruijn_compact_batch_device(int32_t n_seqs, const char* bases, const uint8_t* quals, const int64_t* seq_off,
                                     const uint8_t* mapq, int32_t n_windows, const dv_debruijn_window* windows,
                                     const dv_debruijn_options* options, void* stream,
                                     dv_debruijn_compact_result** out, dv_debruijn_compact* arrays);
typedef struct dv_debruijn_device_stats {
  int64_t windows;           /* windows asked for */
  int64_t windows_on_host;   /* of them over a limit, or overflowing at run time: built by the host code */
  int64_t kmers;             /* k-mer occurrences hashed on the device, summed over the k values tried */
  int64_t k_tries;           /* k values visited, summed over windows */
  int64_t launches;          /* kernel launches */
  int64_t windows_rejected;  /* dv_realign_regions_device only: device graphs dv_debruijn_from_compact's checks
                                refused (rebuilt on the host); must stay 0 */
} dv_debruijn_device_stats;
/* What the calling thread's last dv_debruijn_compact_batch_device or dv_realign_regions_device did with the
 * assembly (all zero when the latter ran it on the host: DV_REALIGN_DEVICE_ASSEMBLY unset). */
int dv_debruijn_device_last_stats(dv_debruijn_device_stats* out);
/* The graph dv_debruijn_build returns, rebuilt from one window's compact form (n_vertices / n_edges entries of the
 * arrays above) and pruned as dv_debruijn_build prunes; the reads as for dv_debruijn_build.  *out = NULL for k = 0.
 * The compact form is validated before anything is indexed by it -- occurrences inside their sequences, edge
 * endpoints in range, the reference's vertices 0 .. |ref| - k in order, both lists sorted by occurrence -- and a
 * malformed one is DV_ERR_BAD_INPUT. */
int dv_debruijn_from_compact(const char* ref, int64_t ref_len, const uint8_t* bases, const uint8_t* quals,
                             int64_t n_bases, const uint32_t* read_seq_off, const uint8_t* read_mapq,
                             int32_t n_table_reads, const int32_t* reads, int32_t n_reads,
                             const dv_debruijn_options* options, int32_t k, int32_t n_vertices,
                             const int32_t* vertex_seq, const int32_t* vertex_pos, int32_t n_edges,
                             const int32_t* edge_from, const int32_t* edge_to, const int32_t* edge_weight,
                             const int32_t* edge_is_ref, const int32_t* edge_seq, const int32_t* edge_pos,
                             dv_debruijn_graph** out);

/* The candidate haplotypes of many windows in one call: what dv_debruijn_build + dv_debruijn_haplotypes give per
 * window, as text.  The arguments are dv_debruijn_compact_batch's.  status[w] is 0: the window's haplotypes follow,
 * exactly candidate_haplotypes()'s and in its order ([reference] when the graph has one walk); 1: no graph
 * (dv_debruijn_build returns NULL; k[w] = 0); 2: more than max_num_paths walks, no haplotypes.  Window w's haplotypes
 * are numbers [hap_first[w], hap_first[w + 1]); haplotype h is hap_text[hap_off[h], hap_off[h + 1]). */
typedef struct dv_debruijn_paths {     /* views into the result; valid until dv_debruijn_paths_free */
  const int32_t* k;                /* [n_windows] the winning k, 0 for no graph */
  const int32_t* status;           /* [n_windows] DV_DEBRUIJN_PATHS_* */
  const int32_t* hap_first;        /* [n_windows + 1] into hap_off */
  const int64_t* hap_off;          /* [n_haps + 1] into hap_text */
  const char* hap_text;
} dv_debruijn_paths;
#define DV_DEBRUIJN_PATHS_OK 0
#define DV_DEBRUIJN_PATHS_NO_GRAPH 1
#define DV_DEBRUIJN_PATHS_TOO_MANY 2
typedef struct dv_debruijn_paths_result dv_debruijn_paths_result;
/* Host code: DeBruijnGraph::build and candidate_haplotypes per window.  The reference of the device form. */
int dv_debruijn_paths_batch(int32_t n_seqs, const char* bases, const uint8_t* quals, const int64_t* seq_off,
                            const uint8_t* mapq, int32_t n_windows, const dv_debruijn_window* windows,
                            const dv_debruijn_options* options, dv_debruijn_paths_result** out,
                            dv_debruijn_paths* arrays);
void dv_debruijn_paths_free(dv_debruijn_paths_result* r);
/* The same from the device (csrc/debruijn.hip): one upload, the graph launch and one paths launch behind it with a
 * workgroup per window each -- pruning, the count of source -> sink walks and the walks' text in lexicographic order
 * --, one download of per-window headers and haplotype slices (no vertex or edge pools) and one synchronisation on
 * `stream` (NULL = a non-blocking stream the library owns); identical arrays.  Not an error, but computed by the host
 * code inside the call and counted in windows_on_host: a window the graph kernel hands back (the limits above), a
 * window whose haplotypes' text passes DV_DEBRUIJN_DEVICE_MAX_HAP_BYTES, and every window of a call with
 * disable_graph_pruning set or max_num_paths above DV_DEBRUIJN_DEVICE_MAX_PATHS.  Errors as
 * dv_debruijn_compact_batch_device; DV_ERR_NO_DEVICE only when there is device work. */
#define DV_DEBRUIJN_DEVICE_MAX_PATHS 1024
#define DV_DEBRUIJN_DEVICE_MAX_HAP_BYTES 262144
int dv_debruijn_paths_batch_device(int32_t n_seqs, const char* bases, const uint8_t* quals, const int64_t* seq_off,
                                   const uint8_t* mapq, int32_t n_windows, const dv_debruijn_window* windows,
                                   const dv_debruijn_options* options, void* stream, dv_debruijn_paths_result** out,
                                   dv_debruijn_paths* arrays);
typedef struct dv_debruijn_paths_stats {
  int64_t windows;           /* windows asked for */
  int64_t windows_on_host;   /* of them computed by the host code (see above) */
  int64_t paths;             /* haplotypes the device produced */
  int64_t hap_bytes;         /* their text */
  int64_t launches;          /* kernel launches, the graph kernel's included */
  int64_t bytes_down;        /* size of the download */
} dv_debruijn_paths_stats;
/* What the calling thread's last dv_debruijn_paths_batch_device or dv_realign_regions_device did with the paths (all
 * zero when the latter did not use them: DV_REALIGN_DEVICE_PATHS unset). */
int dv_debruijn_paths_last_stats(dv_debruijn_paths_stats* out);

/* ---- the window realigner over many regions in one call (host only, threaded) -----
 * Replaces the body of Realigner.realign_reads (deepvariant/realigner/realigner.py:795-855) for a
 * BATCH of calling regions whose candidate windows are already selected: per window the reads
 * that overlap it are assembled (call_debruijn_graph, :703-738; windows whose only haplotype is
 * the reference are dropped), every read joins the assembled window it shares most bases with
 * (assign_reads_to_assembled_regions, :596-619; the first such window on ties), and each
 * window's reads are realigned against its haplotypes padded with the reference out to the
 * reads' span + ref_align_margin (call_fast_pass_aligner, :740-793; FastPassAligner::AlignReads,
 * deepvariant/realigner/fast_pass_aligner.cc:131-177).  The reference runs this window by
 * window from Python, one make_examples process per core; here the (region, window) tasks of
 * the whole batch are spread over `n_threads` host threads inside one call, and nothing but
 * arrays crosses the boundary.  Results are those of the per-window entry points above. */
typedef struct dv_realign_region {
  /* the region's reads: dv_batch's arrays (one row per read, in the caller's order) */
  const uint8_t* bases;
  const uint8_t* quals;
  int64_t n_bases;
  const uint32_t* read_seq_off;    /* [n_reads + 1] */
  const uint8_t* read_mapq;        /* [n_reads] */
  const int64_t* read_start;       /* [n_reads] alignment start */
  const int64_t* read_end;         /* [n_reads] alignment end, exclusive (ReadRange) */
  int32_t n_reads;
  int32_t n_windows;               /* candidate windows, sorted; each inside the contig and */
  const int64_t* window_start;     /*   no longer than ws_config.max_window_size (the caller's */
  const int64_t* window_end;       /*   filter, realigner.py:717-722) */
  const char* ref;                 /* reference bases [ref_start, ref_start + ref_len): must cover */
  int64_t ref_start;               /*   every read and window +- ref_align_margin, clipped to */
  int64_t ref_len;                 /*   [0, contig_len) */
  int64_t contig_len;
} dv_realign_region;

typedef struct dv_realign_options {
  dv_debruijn_options dbg;
  dv_aligner_options aln;          /* read_size, ref_prefix_len, ref_suffix_len are set per window */
  int32_t ref_align_margin;        /* _REF_ALIGN_MARGIN, realigner.py:263 (20) */
  int32_t n_threads;               /* <= 0: one per hardware thread, at most 16 */
} dv_realign_options;

typedef struct dv_realign_output {   /* views into the result; valid until dv_realign_result_free */
  const int64_t* region_row_off;     /* [n_regions + 1]: region g's rows are [off[g], off[g + 1]) below */
  const int32_t* order;              /* rows of the region in the order realign_reads returns its reads:
                                        first the ones no window claimed, then window by window */
  const int32_t* status;             /* per row (input order): 0 alignment kept, 1 new alignment */
  const int64_t* position;           /* new alignment start, status 1 */
  const int64_t* cigar_off;          /* [rows + 1] into `cigar`; empty unless status 1 */
  const uint32_t* cigar;             /* (length << 4 | op) words */
  const int32_t* region_assembled_off;   /* [n_regions + 1] into the assembled-window arrays */
  const int32_t* assembled_window;   /* index in the region's window list */
  const int32_t* assembled_hap_off;  /* [n_assembled + 1] into the haplotype list */
  const int64_t* hap_text_off;       /* [n_haplotypes + 1] into hap_text */
  const char* hap_text;              /* CandidateHaplotypes.haplotypes, sorted per window */
} dv_realign_output;

typedef struct dv_realign_result dv_realign_result;
int dv_realign_regions(const dv_realign_region* regions, int32_t n_regions, const dv_realign_options* options,
                       dv_realign_result** out, dv_realign_output* arrays);
void dv_realign_result_free(dv_realign_result* r);
/* The same call with the local alignments of phase 2 on the device: the (haplotype, reference) and
 * (read, haplotype) pairs of every window of the batch go through ONE dv_local_align_pairs_device-style
 * launch on `stream` (NULL = the library's own), between a host loop that prepares the windows and one
 * that finishes them.  `out` / `arrays` are identical, array by array, to dv_realign_regions' and are
 * freed by dv_realign_result_free.  `stats` (may be NULL) receives what the device did.  Opt-in:
 * dv_realign_regions itself never touches a device.  DV_ERR_NO_DEVICE without a GPU.
 * DV_REALIGN_DEVICE_FASTPASS=1 in the environment, read at each call, also moves the fast pass of every
 * window there (dv_fast_pass_batch_device's kernel: one more launch per call, no k-mer index on the host);
 * unset or 0 it runs on the host threads.  Results are identical either way; `stats` keeps counting the
 * sweep kernel only, dv_fast_pass_device_last_stats reports the fast pass.
 * DV_REALIGN_DEVICE_ASSEMBLY=1, read at each call as well, moves phase 1's graph building there: the windows of all
 * regions go through one dv_debruijn_compact_batch_device-style launch, and the host threads prune and enumerate
 * from the compact graphs (dv_debruijn_from_compact's code); unset or 0 each window is built on a host thread.
 * dv_debruijn_device_last_stats reports it.
 * DV_REALIGN_DEVICE_PATHS=1, read at each call and honoured only together with DV_REALIGN_DEVICE_ASSEMBLY=1, also
 * prunes and enumerates there (dv_debruijn_paths_batch_device's kernels): the host threads only compare a window's
 * haplotypes with its reference, and build the windows the device hands back.  dv_debruijn_paths_last_stats reports
 * it.
 * DV_REALIGN_DEVICE_FINISH=1, read at each call and honoured only together with DV_REALIGN_DEVICE_TRACEBACK=1, also
 * finishes the alignments there (dv_align_windows_batch_device's finish kernels, behind the sweep launch whose result
 * stays on the device): the host threads make the text form and run FastPassAligner::finish_alignments only for the
 * windows the device hands back.  dv_realign_finish_last_stats reports it. */
int dv_realign_regions_device(const dv_realign_region* regions, int32_t n_regions, const dv_realign_options* options,
                              void* stream, dv_realign_result** out, dv_realign_output* arrays,
                              dv_realign_device_stats* stats);

/* ---- read phasing for the long-read path (host only) ---------------------------
 * Replaces deepvariant/direct_phasing.{h,cc} (DirectPhasing::PhaseReads / GetPhasedVariants;
 * python binding deepvariant/python/direct_phasing_pybind.cc).  A candidate is a
 * DeepVariantCall reduced to what phasing reads: variant.start / end and, per called allele
 * (allele_support_ext key, UNCALLED_ALLELE left out) plus one is_ref entry for
 * ref_support_ext, the supporting reads as indices into the reads being phased (-1: a read
 * that is not among them) with their is_low_quality flags. */
typedef struct dv_phasing_allele {
  int64_t bases_off;        /* into `bases` */
  int32_t bases_len;
  int32_t is_ref;
  int64_t support_off;      /* into support_reads / support_low_quality */
  int32_t n_support;
  int32_t reserved;
} dv_phasing_allele;

typedef struct dv_phasing_candidate {
  int64_t start, end;
  int32_t allele_off, n_alleles;   /* into `alleles` */
} dv_phasing_candidate;

/* read_phases[n_reads] receives 0 / 1 / 2 (PhaseReads' return value).  Optional outputs, per
 * allele-table entry: allele_phases (-1 = the allele is not a vertex of the graph) and
 * allele_flags (1 = first site of its phase block) -- what GetPhasedVariants reads -- and
 * the graph as text (GraphViz()).  Candidates must be strictly ordered by start. */
int dv_phase_reads(const dv_phasing_candidate* candidates, int32_t n_candidates, const dv_phasing_allele* alleles,
                   int32_t n_alleles, const char* bases, int64_t n_bases, const int32_t* support_reads,
                   const uint8_t* support_low_quality, int64_t n_support, int32_t n_reads,
                   int32_t min_alleles_to_phase, int32_t* read_phases, int32_t* allele_phases,
                   uint8_t* allele_flags, char* graphviz, int32_t graphviz_cap);

/* ---- the same for a batch of regions, from arrays (csrc/phasing.hip) -------------
 * The candidate, allele, bases and support arrays are dv_phase_reads' layouts concatenated over the regions;
 * allele_off, bases_off and support_off are absolute.  A region names its slices; its candidates' alleles and
 * their support must lie inside them.  read_phases[first_read .. first_read + n_reads) receives the region's
 * reads; allele_phases / allele_flags are written at the alleles of the region's candidates.  Nothing else is
 * written. */
typedef struct dv_phasing_region {
  int32_t candidate_off, n_candidates;   /* into `candidates` */
  int32_t allele_off, n_alleles;         /* into `alleles` */
  int64_t support_off, n_support;        /* into support_reads / support_low_quality */
  int64_t first_read;                    /* into read_phases */
  int32_t n_reads;
  int32_t reserved;
} dv_phasing_region;

typedef struct dv_phasing_stats {
  int64_t regions;
  int64_t regions_on_host;    /* outside the device limits below: dv_phase_reads_batch_device phased them with
                                 the host code inside the call; dv_phase_reads_batch only counts them */
  int64_t sites_in_graphs;    /* sites that passed the candidate filter */
  int64_t vertices;
  int64_t combinations;       /* (to-pair, from-pair) combinations the kernel scored; 0 from the host entry */
  int64_t launches;           /* 1 when a region went to the device, else 0 */
} dv_phasing_stats;

/* A region goes to the device when it has at most DV_PHASING_DEVICE_MAX_READS reads (the two live positions'
 * read sets are bitmaps in LDS), no site with more than DV_PHASING_DEVICE_MAX_VERTICES graph vertices, distinct
 * vertex texts within every site and no read (known, not low quality) listed twice under one site. */
#define DV_PHASING_DEVICE_MAX_READS 1024
#define DV_PHASING_DEVICE_MAX_VERTICES 8

/* Host code: dv_phase_reads' checker region by region.  Candidates of a region not strictly ordered by start,
 * or a read index >= n_reads: DV_ERR_BAD_INPUT naming the smallest such region.  Null pointers, negative counts
 * and slices outside their tables: DV_ERR_INVALID_ARGUMENT.  An error leaves the outputs untouched.
 * allele_phases, allele_flags and stats may be NULL. */
int dv_phase_reads_batch(const dv_phasing_region* regions, int32_t n_regions, const dv_phasing_candidate* candidates,
                         int32_t n_candidates, const dv_phasing_allele* alleles, int32_t n_alleles, const char* bases,
                         int64_t n_bases, const int32_t* support_reads, const uint8_t* support_low_quality,
                         int64_t n_support, int64_t n_reads_total, int32_t min_alleles_to_phase, int32_t* read_phases,
                         int32_t* allele_phases, uint8_t* allele_flags, dv_phasing_stats* stats);
/* The same on the device: one upload, ONE launch (a workgroup per region), one download and one synchronisation
 * on `stream` (NULL = a non-blocking stream the library owns); identical arrays.  A region outside the limits is
 * not an error: the host code phases it inside the same call.  No region or no candidate at all is DV_OK without
 * a device; no device is DV_ERR_NO_DEVICE (there is no CPU fallback). */
int dv_phase_reads_batch_device(const dv_phasing_region* regions, int32_t n_regions,
                                const dv_phasing_candidate* candidates, int32_t n_candidates,
                                const dv_phasing_allele* alleles, int32_t n_alleles, const char* bases, int64_t n_bases,
                                const int32_t* support_reads, const uint8_t* support_low_quality, int64_t n_support,
                                int64_t n_reads_total, int32_t min_alleles_to_phase, int32_t* read_phases,
                                int32_t* allele_phases, uint8_t* allele_flags, dv_phasing_stats* stats, void* stream);
/* What the calling thread's last dv_phase_reads_batch_device did. */
int dv_phase_device_last_stats(dv_phasing_stats* out);

/* ---- alt-aligned channel merge (device) --------------------------------------
 * FillPileupArray's diff_channels / base_channels modes (deepvariant/pileup_image_native.h:
 * 246-271) on images that stay in HBM: `images` holds the examples followed, from
 * `scratch_offset`, by scratch images of `scratch_image_bytes` each (the alt images, items of
 * the same dv_encode_batch launch); per entry the two channels first_alt_channel, +1 of rows
 * [first_row, first_row + rows) of one example receive channel `source_channel` (5 or 0) of
 * scratch image scratch_alt1 and scratch_alt2 (alt 1 again when scratch_alt2 < 0). */
typedef struct dv_alt_merge_entry {
  int64_t example;
  int32_t first_row, rows;
  int64_t scratch_alt1, scratch_alt2;
} dv_alt_merge_entry;

int dv_merge_alt_channels(uint8_t* images, uint64_t scratch_offset, uint64_t example_bytes,
                          uint64_t scratch_image_bytes, int32_t width, int32_t channels,
                          int32_t first_alt_channel, int32_t source_channel,
                          const dv_alt_merge_entry* entries, int32_t n_entries, void* stream);

/* ---- allele counting (device) -------------------------------------------------
 * Replaces the per-read loop around AlleleCounter::Add for one region
 * (deepvariant/allelecounter.cc:873-979 with MakeIndelReadAllele :402-469, GetPrevBase
 * :386-400, CanBasesBeUsed :206-229, AddReadAlleles :471-543; constructed as in :349-369).
 * The reads come as the read-table fields of a dv_batch (host or device memory); the result
 * is AlleleCount's content per interval position: ref_supporting_read_count plus one event
 * per non-reference read allele (the host builds read_alleles / allele sums from events:
 * deepvariant_amd/allelecounter.py).  Not produced: methylation fields, REFERENCE read
 * alleles of track_ref_reads, sample_alleles. */
typedef struct dv_allele_counter_options {
  int64_t interval_start, interval_end;             /* AlleleCounter's range (counts are reported here) */
  int64_t reads_interval_start, reads_interval_end; /* full_range (:349-369); pass the interval again if unused */
  const char* ref_bases;                            /* reference of [ref_start, ref_start + n_ref_bases): must cover the
                                                       reads interval; indels that reach outside it are an error */
  int64_t ref_start, n_ref_bases;
  int64_t contig_n_bases;                           /* RefBases validity (:371-384); 0 = end of the window */
  int32_t min_mapping_quality, min_base_quality;    /* AlleleCounterOptions.read_requirements */
  int32_t keep_legacy_behavior;                     /* AlleleCounterOptions.keep_legacy_behavior */
  /* AlleleCounterOptions.track_ref_reads + the constructor's candidate_positions (absolute, any order):
   * at those positions reference-supporting reads are reported too, as events of type 1 (REFERENCE),
   * so that the caller can name them (ref_support_ext, read phasing); allelecounter.cc:504-512 */
  int32_t track_ref_reads;
  const int64_t* candidate_positions;
  int32_t n_candidate_positions;
} dv_allele_counter_options;

typedef struct dv_allele_event {   /* one ReadAllele that AddReadAlleles stores in read_alleles */
  int32_t position;      /* offset in the interval */
  uint32_t read;         /* index in the read table */
  uint32_t read_offset;  /* SUBSTITUTION: the base; INSERTION / SOFT_CLIP: first inserted base; DELETION: next read base */
  uint32_t length_type;  /* bits 0-27: operation length (1 for substitutions; a BAM CIGAR length has 28 bits,
                            so long HiFi / ONT soft clips and deletions are exact);
                            bits 28-30: AlleleType: 2 SUBSTITUTION, 3 INSERTION, 4 DELETION, 5 SOFT_CLIP;
                            1 REFERENCE (track_ref_reads, candidate positions only; read_offset = the base);
                            bit 31: Allele.is_low_quality */
} dv_allele_event;

typedef struct dv_allele_counts dv_allele_counts;  /* owns the host copies of the result */

int dv_count_alleles(const dv_batch* reads, const dv_allele_counter_options* options, dv_allele_counts** out,
                     void* stream);
/* The same for n regions (a region driver's batch of calling regions, each with its own read
 * table and options): every region's arrays travel in one pinned staging image, the kernels are
 * queued back to back and the stream is synchronised twice for the whole batch instead of twice
 * per region.  out[k] receives region k's result (each freed with dv_allele_counts_free); on an
 * error no result is left allocated. */
int dv_count_alleles_batch(int32_t n, const dv_batch* const* reads, const dv_allele_counter_options* const* options,
                           dv_allele_counts** out, void* stream);
/* Events are sorted by (position, read, read_offset) = the order AddReadAlleles stores them
 * for one position.  Returns the interval length. */
int dv_allele_counts_arrays(const dv_allele_counts* c, const int32_t** ref_supporting_read_count,
                            const dv_allele_event** events, uint32_t* n_events, int32_t* n_reads_counted);
void dv_allele_counts_free(dv_allele_counts* c);

/* ---- gVCF reference-confidence blocks (device) ----------------------------------
 * VariantCaller.make_gvcfs(allele_counter.summary_counts(left_padding, right_padding)) of the
 * reference's deepvariant/variant_caller.py, computed next to the allele counter from the counts
 * where they lie on the device; only the merged block records come back.  Per site of the
 * interval (padding removed): n_ref = ref_supporting_read_count, n_total = TotalAlleleCounts
 * (read alleles that are neither low quality nor REFERENCE, the later allele of one read key at
 * one position standing, plus n_ref); deeper than max_cache_coverage the counts are rescaled
 * (n_ref = ceil(n_ref / (1.0 * n_total) * M) in IEEE double, n_total = M) and the site's GQ and
 * likelihoods are looked up in `table`; GQ is quantised by gq_resolution; runs of equal
 * (quantised GQ, has_valid_gl) become one record.  A non-ACGT IUPAC reference base
 * (NRYKMSWBDHV) ends a run and gives no record; any other character is DV_ERR_BAD_INPUT.
 *
 * The table is computed by the caller with the host restatement
 * (deepvariant_amd/variant_calling.py reference_confidence_table): one restatement of the
 * likelihood model, which the device only reads.  It is uploaded when it differs from the last
 * one seen on this host thread and device. */
typedef struct dv_gvcf_site {
  double likelihoods[3];   /* normalised log10 genotype likelihoods (hom-ref, het, hom-alt) */
  int32_t gq;              /* raw GQ */
  int32_t has_valid_gl;    /* max(likelihoods) == likelihoods[0] */
} dv_gvcf_site;

typedef struct dv_gvcf_options {
  double p_error;               /* what `table` was computed with (0.001 in the reference) */
  int32_t max_gq;               /* likewise (50) */
  int32_t gq_resolution;        /* gvcf_gq_binsize (5), >= 1 */
  int32_t max_cache_coverage;   /* M: the table covers 0 <= n_ref <= n_total <= M */
  int32_t include_med_dp;       /* compute MED_DP */
  int32_t left_padding, right_padding;   /* sites are [interval_start + left, interval_end - right) */
  const dv_gvcf_site* table;    /* entry n_total * (n_total + 1) / 2 + n_ref */
  int64_t n_table;              /* (M + 1) * (M + 2) / 2 */
} dv_gvcf_options;

typedef struct dv_gvcf_block {  /* one gVCF record: Variant(start, end, ref, ['<*>']) with one call */
  int64_t start, end;           /* absolute; end exclusive */
  double likelihoods[3];        /* genotype_likelihood: the first site's */
  int32_t gq;                   /* info GQ: the smallest raw GQ of the block */
  int32_t min_dp;               /* MIN_DP: the smallest n_total */
  int32_t med_dp;               /* MED_DP: int(statistics.median(n_total)); -1 unless include_med_dp */
  uint8_t ref_base;             /* reference_bases: the first site's base */
  uint8_t has_valid_gl;
  uint8_t reserved[2];
} dv_gvcf_block;

typedef struct dv_gvcf_blocks dv_gvcf_blocks;

/* dv_count_alleles_batch plus the gVCF blocks of every region, from the same counts in the same
 * device pass (no further synchronisation).  read_keys[k] (may be NULL, as may read_keys):
 * region k's read-key id per read (equal ids = one key of read_alleles, e.g. the supplementary
 * alignments of a read); NULL = every read its own key.  blocks_out[k] receives region k's
 * records (each freed with dv_gvcf_blocks_free); counts_out as for dv_count_alleles_batch.  On an
 * error no result is left allocated. */
int dv_count_alleles_gvcf_batch(int32_t n, const dv_batch* const* reads, const dv_allele_counter_options* const* options,
                                const int32_t* const* read_keys, const dv_gvcf_options* gvcf,
                                dv_allele_counts** counts_out, dv_gvcf_blocks** blocks_out, void* stream);
/* -> the number of records; *blocks points at them (owned by `b`). */
int64_t dv_gvcf_blocks_arrays(const dv_gvcf_blocks* b, const dv_gvcf_block** blocks);
void dv_gvcf_blocks_free(dv_gvcf_blocks* b);

/* ---- candidate caller (device) --------------------------------------------------
 * VariantCaller::CallsFromAlleleCounter / CallPositionsFromAlleleCounts of the reference's
 * deepvariant/variant_calling.cc:365-382 and variant_calling_multisample.cc:940-1004, single-sample form
 * (SelectAltAlleles / IsGoodAltAllele :232-258 over SumAlleleCounts / TotalAlleleCounts,
 * allelecounter.cc:78-203), computed behind the allele counter from the counts and events where they
 * lie on the device.  Per interval position the later event of one read key stands; the standing
 * events are grouped into alleles by (type, text) -- substitution: the base; deletion: length and
 * anchor base; insertion / soft clip: length, anchor base and the inserted read bases -- low-quality
 * events belonging to their group without counting; total = good non-REFERENCE events +
 * ref_supporting_read_count; an allele is selected when it is neither REFERENCE nor SOFT_CLIP,
 * count >= min_count_* and (1.0 * count) / total >= (double)min_fraction_* (the thresholds are proto
 * `float` fields: the comparison is IEEE double against the float32 value), on an A/C/G/T reference
 * base.  Not restated: multi-sample filtering, complex alleles, reference-site sampling, methylation. */
typedef struct dv_candidate_options {
  int32_t min_count_snps, min_count_indels;       /* VariantCallerOptions, >= 0 */
  float min_fraction_snps, min_fraction_indels;   /* >= 0 */
  int32_t track_ref_reads;   /* VariantCallerOptions.track_ref_reads: REFERENCE events (counter options'
                                track_ref_reads) take part in the read-key rule and get "uncalled" words either
                                way; the flag travels for the host, which names them only when it is set */
  int32_t positions_only;    /* CallPositionsFromAlleleCounts: only the sites' offsets are produced; no
                                events, counts, allele records or event words come back */
} dv_candidate_options;

typedef struct dv_candidate_site {   /* one position CallVariant returns a call for, in position order */
  int32_t offset;         /* position - interval_start */
  int32_t ref_count;      /* ref_supporting_read_count (AD[0]) */
  int32_t total;          /* TotalAlleleCounts (DP) */
  int32_t first_allele;   /* index of the site's first record among the region's allele records */
  int32_t n_alleles;      /* selected alleles, >= 1 */
} dv_candidate_site;

typedef struct dv_candidate_allele {   /* one selected alternate allele */
  uint32_t length_type;   /* as dv_allele_event.length_type, low-quality bit clear */
  int32_t count;          /* good-quality reads that carry it */
  uint32_t read, read_offset;   /* a representative event (the first in event order): where its text is */
} dv_candidate_allele;

#define DV_CANDIDATE_EVENT_UNCALLED (-1)      /* the event stands, its allele was not selected (UNCALLED_ALLELE) */
#define DV_CANDIDATE_EVENT_OVERWRITTEN (-2)   /* a later event of the same read key replaced it */

typedef struct dv_candidates dv_candidates;   /* owns the host copies of one region's result */

/* dv_count_alleles_batch plus the candidates of every region from the same counts in the same device
 * pass (no further synchronisation), and -- with `gvcf` / blocks_out, both optional -- the gVCF records
 * of dv_count_alleles_gvcf_batch as well.  read_keys as there.  candidates_out[k] receives region k's
 * sites (freed with dv_candidates_free); counts_out as for dv_count_alleles_batch.  With
 * positions_only, counts_out may be NULL and is left untouched, and `gvcf` must be NULL.  Negative
 * thresholds are DV_ERR_INVALID_ARGUMENT; on an error no result is left allocated. */
int dv_call_candidates_batch(int32_t n, const dv_batch* const* reads, const dv_allele_counter_options* const* options,
                             const int32_t* const* read_keys, const dv_candidate_options* candidate_options,
                             const dv_gvcf_options* gvcf, dv_allele_counts** counts_out, dv_gvcf_blocks** blocks_out,
                             dv_candidates** candidates_out, void* stream);
/* -> the number of sites.  event_words[i] belongs to event i of dv_allele_counts_arrays: the ordinal
 * (0 .. n_alleles - 1) of its site's selected allele that the event supports, or one of the two
 * negative codes above; n_events is 0 with positions_only. */
int64_t dv_candidates_arrays(const dv_candidates* c, const dv_candidate_site** sites,
                             const dv_candidate_allele** alleles, int32_t* n_alleles, const int32_t** event_words,
                             uint32_t* n_events);
void dv_candidates_free(dv_candidates* c);

/* ---- realigner window selection (device) ----------------------------------------
 * select_windows of the reference's deepvariant/realigner/window_selector.py:40-238 over
 * VariantReadsWindowSelectorCandidates / AlleleCountLinearWindowSelectorCandidates
 * (window_selector.cc:101-207), computed behind the allele counter from the counts and events where
 * they lie on the device.  Per interval position the later event of one read key stands (as for the
 * candidate caller).  A standing event at offset i covers [i, i+1) (substitution, REFERENCE),
 * [i+1-n, i+1+n) (insertion or soft clip of n bases) or [i+1, i+1+n) (deletion of n bases), clipped
 * to the interval.
 *   VARIANT_READS: a good-quality non-REFERENCE standing event adds 1 over its footprint when its
 *     allele (type, text) has >= min_allele_support good events and, with
 *     enable_strict_insertion_filter and an insertion of at most one base,
 *     (double)((float)count / (float)total) >= 0.08, total = the position's good non-REFERENCE
 *     standing events + ref_supporting_read_count.  Candidate: min <= count <= max.
 *   ALLELE_COUNT_LINEAR: float32, summed in the reference's order, one round-to-nearest operation
 *     per step: score[j] = (float)bias; + coeff[type] for every standing event (low-quality and
 *     REFERENCE ones included) of positions i < j that covers j, in ascending i and within one
 *     position in the order of the first event of each read key; + (float)ref_count[j] *
 *     coeff_reference; + the same for positions i >= j.  Candidate: (double)score > decision_boundary.
 * Candidates more than 2 * min_windows_distance apart start a new window; a window is
 * [first - d, last + d) in contig coordinates, not clamped to the contig. */
#define DV_WINDOW_MODEL_VARIANT_READS 1
#define DV_WINDOW_MODEL_ALLELE_COUNT_LINEAR 2

typedef struct dv_window_options {
  int32_t model_type;                 /* DV_WINDOW_MODEL_* */
  int32_t min_num_supporting_reads, max_num_supporting_reads;   /* VARIANT_READS; max >= min whatever the model */
  int32_t min_allele_support;
  int32_t enable_strict_insertion_filter;
  float bias, coeff_soft_clip, coeff_substitution, coeff_insertion, coeff_deletion, coeff_reference;
  int32_t min_windows_distance;       /* d, >= 0 */
  double decision_boundary;
  int32_t want_debug;                 /* also bring home the candidate mask and the scores (for tests) */
  int32_t reserved;
} dv_window_options;

typedef struct dv_windows dv_windows;   /* owns the host copies of one region's result */

/* The windows of every region from one device pass behind the counting kernels.  read_keys as for
 * dv_count_alleles_gvcf_batch.  windows_out[k] receives region k's windows (freed with
 * dv_windows_free).  counts_out may be NULL: then neither counts nor events come home, only the
 * windows; otherwise it is filled as by dv_count_alleles_batch.  An unknown model type, max < min
 * or a negative distance is DV_ERR_INVALID_ARGUMENT; on an error no result is left allocated. */
int dv_select_windows_batch(int32_t n, const dv_batch* const* reads, const dv_allele_counter_options* const* options,
                            const int32_t* const* read_keys, const dv_window_options* window_options,
                            dv_allele_counts** counts_out, dv_windows** windows_out, void* stream);
/* -> the number of windows; starts / ends in contig coordinates, end exclusive.  With want_debug,
 * candidate_mask holds one bit per interval position (bit p & 31 of word p >> 5) and scores one word
 * per position: the float32 score, or for VARIANT_READS the count as int32; both NULL otherwise. */
int64_t dv_windows_arrays(const dv_windows* w, const int64_t** starts, const int64_t** ends,
                          const uint32_t** candidate_mask, const uint32_t** scores);
void dv_windows_free(dv_windows* w);

/* How the counting in front of every batch entry point above was launched.  A batch uploads the host-resident
 * regions that have reads and an interval in one image ("batched"); by default each of them is then counted by a
 * launch of its own, ceil(n_reads / 64) workgroups each.  With DV_COUNT_ONE_LAUNCH=1 in the environment (read at
 * every call; off by default) one launch covers them all: the same workgroups in one grid, each finding its region
 * by bisection of a block prefix that travels with the upload.  The switch changes no result: counts are integer
 * atomic sums, and the events, whose raw order varies from run to run either way, come home sorted by
 * (position, read, read_offset).  Regions that are not batched (a device-resident table) and regions whose events
 * overflow the batch's first guess are counted by the one-region kernel afterwards, with or without the switch. */
typedef struct dv_count_batch_stats {
  int32_t regions;           /* n of the call */
  int32_t regions_batched;   /* counted by the batch's own launches */
  int32_t regions_alone;     /* counted by a one-region launch: not batched, or overflowed and repeated */
  int32_t count_launches;    /* counting launches for the batched regions: regions_batched, or 1 with the switch */
  int64_t count_workgroups;  /* workgroups of those launches together */
} dv_count_batch_stats;
/* What the calling thread's last dv_count_alleles_batch, dv_count_alleles_gvcf_batch, dv_call_candidates_batch or
 * dv_select_windows_batch did (all zero before the first).  A null pointer is DV_ERR_INVALID_ARGUMENT. */
int dv_count_batch_last_stats(dv_count_batch_stats* out);

/* CRC32C (Castagnoli) as used by TFRecord framing
 * (third_party/nucleus/io/example_writer.cc:88-104 via tensorflow::io::RecordWriter). */
uint32_t dv_crc32c(const uint8_t* data, size_t n);

/* ------------------------------------------------------------------ model */

/* Inception-v3 classifier as instantiated by
 * deepvariant/keras_modeling.py:246-336 (tf_keras InceptionV3,
 * include_top=False, pooling='avg') + Dense(3, softmax) head (:46-67), for
 * input [height, width, channels] uint8. */
typedef struct dv_model_desc {
  int32_t height;
  int32_t width;
  int32_t channels;
  int32_t num_classes; /* 3 */
  int32_t max_batch;   /* activations are sized for this many examples (<= 8192; ~6 MB of HBM each at 100x221) */
} dv_model_desc;

int dv_model_create(const dv_model_desc* desc, int device, dv_model** out);
void dv_model_destroy(dv_model* m);

/* Number of fp32 values dv_model_load_weights expects and, per layer i of
 * dv_model_num_layers(), its slice: conv kernel HWIO (kh*kw*cin*cout) then BN
 * beta, moving_mean, moving_variance (cout each); the last layer is the Dense
 * kernel [2048, num_classes] + bias.  Layer order = tf_keras CONSTRUCTION
 * order (applications/inception_v3.py).  That is NOT the
 * checkpoint's `layer_with_weights-N` numbering, which follows Keras'
 * depth-sorted `model.layers`: a TensorFlow checkpoint is mapped by variable
 * name and shape by the host importer (deepvariant_amd/keras_layout.py,
 * call_variants.import_keras_checkpoint), never by position. */
int64_t dv_model_num_params(const dv_model* m);
/* Multiply-accumulates of the 94 convolutions for ONE example of the model's input
 * shape (padding taps included, as in every FLOP count of this architecture): the
 * algorithmic work bench.py prices the conv kernels with. */
int64_t dv_model_conv_macs(const dv_model* m);
int dv_model_num_layers(const dv_model* m);
int dv_model_layer_info(const dv_model* m, int layer, int32_t* kh, int32_t* kw,
                        int32_t* cin, int32_t* cout, int64_t* param_offset);

/* Folds BatchNorm (scale=False, eps=1e-3) into the conv weights, converts to
 * fp16 in the MFMA fragment layout and uploads.  `weights` is host memory.
 * Replaces model.load_weights (deepvariant/call_variants.py:759-762). */
int dv_model_load_weights(dv_model* m, const float* weights, int64_t n);

/* Shift calibration (ABI v7; optional, after dv_model_load_weights with the SAME `weights`).
 * The classifier multiplies fp16 weights by fp16 activations where the reference computes in float32
 * (deepvariant/call_variants.py:913-918).  Both roundings have a per-channel MEAN (the weight
 * error is one fixed draw multiplying activations that are far from zero-mean; constant map regions
 * round identically everywhere); this call measures it on `n_images` example images -- two fp32
 * pipelines on the device, one exact, one with the MFMA kernels' roundings, walked layer by layer
 * (csrc/calib.h) -- and moves each layer's fp32 shift (and the Dense bias) by the difference of the
 * per-channel pre-activation means.  No run-time cost; deterministic for given weights and images;
 * calling it again replaces the previous correction.  Any batch drawn like the inputs the model
 * will see serves (a few hundred pile-ups; tests use OTHER images than the ones they check).
 *   weights  host, the array given to dv_model_load_weights
 *   images   device uint8 [n_images, height, width, channels]
 *   corrections  optional host array [capacity]: the shift corrections in layer order (cout values per
 *                convolution), then num_classes logit corrections; for tests and reports
 * The reference has no counterpart: it keeps float32 end to end. */
int dv_model_calibrate(dv_model* m, const float* weights, int64_t n_weights, const uint8_t* images,
                       int n_images, float* corrections, int64_t capacity);

/* Applies shift corrections measured elsewhere (ABI v7): `corrections` in the layout dv_model_calibrate
 * reports -- cout values per convolution in layer order, then num_classes logit corrections; `n` must be
 * exactly that many.  Replaces any previous correction (the loaded shifts minus these).  For host
 * processes that share one set of weights -- the ranks of `make_examples --ranks_per_gpu R`: one of them
 * calibrates, the others apply its result instead of repeating the measurement on the same GPU. */
int dv_model_apply_corrections(dv_model* m, const float* corrections, int64_t n);

/* Diagnostic (ABI v8): WHERE the fp16 error of the classifier enters.  Runs dv_model_calibrate's two fp32
 * pipelines (csrc/calib.h: R exact, E with the MFMA kernels' rounding points) on `n_images` device images with FIXED
 * shift corrections (`corrections` in dv_model_calibrate's layout, or NULL for none) and returns both pipelines'
 * logits (host, [n_images][num_classes]; logits_r may be NULL: R is skipped).  keep_f32[op] != 0 keeps the output
 * tensor of graph op `op` (0 .. dv_model_num_ops - 1, dv_model_op_label describes each) in float32 in E -- what
 * storing that tensor wider than fp16 would buy; NULL = the product's own rounding points.  flags bit 0: E multiplies
 * the float32 weights (isolates the activation roundings); bit 1: measure the corrections on these images under this
 * plan (the calibration proper; `corrections` must be NULL) and report them in `corrections_out` (optional, the
 * layout of dv_model_calibrate).  The model's state is not changed.  dv_model_num_ops(NULL) is 0; dv_model_op_label
 * writes "kind key=value ..." (at most capacity - 1 characters and a terminating NUL: a short buffer gets a truncated
 * label) and refuses an index outside 0 .. dv_model_num_ops - 1, a NULL buffer or capacity < 1 with
 * DV_ERR_INVALID_ARGUMENT, writing nothing.  tools/r6_tensor_budget.py, tests/test_hip_calib_pipelines.py;
 * no reference counterpart (deepvariant/call_variants.py:913-918 computes in float32 end to end). */
int dv_model_num_ops(const dv_model* m);
int dv_model_op_label(const dv_model* m, int op_index, char* buf, int capacity);
int dv_model_probe_rounding(dv_model* m, const float* weights, int64_t n_weights, const uint8_t* images,
                            int n_images, const uint8_t* keep_f32, int flags, const float* corrections,
                            int64_t n_corrections, float* logits_r, float* logits_e, float* corrections_out);

/* preprocess_images ((x-128)/128, deepvariant/dv_utils.py:343-366) + model
 * forward + softmax (deepvariant/call_variants.py:904-932).
 *   images  device uint8 [n, height, width, channels]
 *   probs   device fp32  [n, num_classes] */
int dv_model_infer(dv_model* m, const uint8_t* images, int n, float* probs,
                   void* stream);

/* Blank-row skipping (ABI v8; on by default for inputs of <= 16 channels).  A pileup image is zero below its last
 * read row (deepvariant/pileup_image_native.cc:405-447 zero-pads every image to `height` rows; a 30x pile-up fills
 * ~40 of 100), and the model normalises zero to the constant -1 (deepvariant/dv_utils.py:343-366): every activation of
 * the stem whose receptive field lies inside those rows equals the all-blank image's response at the same position.
 * dv_model_infer finds each image's last nonzero row (one scan kernel) and the stem kernels copy such tiles from the
 * precomputed response instead of multiplying -- bit-identical to the dense path (tests/test_hip_blank_skip.py), so
 * probabilities are unchanged; only the executed work depends on the images' depth.  `enabled` = 0 runs the dense path
 * (bench.py reports both); the environment variable DV_BLANK_SKIP=0 does the same for a whole process.
 * DV_BLANK_COPY_TILES=1 (read by dv_model_create) makes the two fused stem kernels copy every blank tile their consumer
 * touches, whole, instead of letting stem_b read conv2's blank rows from the response itself and copy one strip per
 * image -- the same bits either way (tests/test_hip_blank_readthrough.py); kept for A/B runs.
 * dv_model_blank_thresholds: what the last forward's scan found for its first n examples, out[k * n + i] with
 * k = 0 first all-zero row, 1..4 the first blank-determined row of conv2 / stem_b / the 3x3 80->192 / its pooled
 * output (bench.py derives the executed FLOPs from them); DV_ERR_UNSUPPORTED when the model does not skip. */
int dv_model_set_blank_skip(dv_model* m, int enabled);

/* Precise mode (ABI v8).  The reference classifies in float32 (deepvariant/call_variants.py:913-918); with fp16 MFMA
 * operands the zero-mean rounding noise of the stored activations puts sigma(dp) of the long-read models' deeper pile-ups
 * at ~2.5e-4, and the largest of a few thousand candidates beyond north_star's 1e-3 on some weight seeds.  In precise
 * mode every fp16 tensor of the 17x17 and 8x8 stages (83 % of that variance; the per-tensor table is
 * profiles/r06_tensor_budget_*.txt) is stored as hi = fp16(x) and lo = fp16(x - hi), and its consumers run their K over
 * both with the same weights: 22-bit activations at twice the MFMA count there, +40 % on the forward.  dv_model_create
 * switches it on for inputs of more than 8 channels (PACBIO, ONT_R104) and off otherwise; the environment variable
 * DV_PRECISE=0 / 1 read at dv_model_create overrides.  Same ABI, same weights, same outputs to within the tolerance. */
int dv_model_is_precise(const dv_model* m);
/* Planner knobs, environment variables read at dv_model_create (A/B runs and tests; the outputs are bit-identical either
 * way): DV_NO_CHAIN=1 keeps every layer of the fused chain family on its own launch, DV_NO_BLOCK35=1 only the 35x35
 * blocks' (block35.hip), DV_NO_MIXED3_FUSE=1 only mixed3's 1x1 -> 3x3 -> 3x3/2 branch (mixed3.hip). */
int dv_model_blank_thresholds(dv_model* m, int n, int32_t* out);

/* dv_model_infer for a caller that KNOWS how many rows of each image are drawn (ABI v8): `rows_used` is a device
 * array int32[n], and the caller promises that in image i every byte of rows >= rows_used[i] + rows_add is zero --
 * what dv_encode_batch's `out_rows` (read rows kept) + the reference band height is for the images it has just drawn.
 * Blank-row skipping then takes its thresholds from the array instead of scanning the images (0.2 ms per 8 K
 * ILLUMINA30 pileups).  NULL = dv_model_infer.  A wrong promise gives wrong probabilities; callers that read images
 * from files (call_variants) use dv_model_infer.  The reference has no counterpart. */
int dv_model_infer_rows(dv_model* m, const uint8_t* images, int n, float* probs, const int32_t* rows_used,
                        int rows_add, void* stream);

/* Intermediate outputs (ABI v8 addition), for integrators of the reference's call_variants --include_debug_info /
 * --activation_layers and for tracing a difference from another implementation to one Inception block.  Names:
 *   mixed0 .. mixed10     Keras InceptionV3's named concat outputs, [h][w][c] per example
 *   mixed9_0, mixed9_1    the 3x3-split concats inside mixed9 and mixed10 (channels 320 .. 1087 of those blocks)
 *   prelogits             the global-average-pooled vector the Dense layer reads, [1][1][2048]
 *   logits                the Dense output before softmax, [1][1][num_classes]
 * Any other name (the unnamed conv2d_N / activation_N layers among them) is DV_ERR_INVALID_ARGUMENT, with the accepted
 * names in dv_last_error.
 * dv_model_output_info: the shape of one example of `name` for this model's input shape.
 * dv_model_infer_outputs: dv_model_infer (the same probabilities, bit for bit: blank-row skipping, calibration and
 * precise mode as there) for n <= max_batch examples, and in addition for every k < n_outputs the DEVICE array
 * outs[k], 16-byte aligned, receives float32 [n][h][w][c] of names[k] (NHWC).  Each name at most once; n above
 * max_batch, a null or misaligned output, an unknown or empty name: DV_ERR_INVALID_ARGUMENT.  n_outputs = 0 is
 * dv_model_infer.  The forward runs with plain launches; the hipGraphs of dv_model_infer are not touched. */
int dv_model_output_info(const dv_model* m, const char* name, int32_t* h, int32_t* w, int32_t* c);
int dv_model_infer_outputs(dv_model* m, const uint8_t* images, int n, float* probs, int n_outputs,
                           const char* const* names, float* const* outs, void* stream);

/* On a non-default stream the forward is captured once per (n, stream) into a hipGraph and
 * replayed; the image / probability pointers are read from a device-side table, so they may
 * change from call to call without a new capture.  Testing hook: captures and replays so far. */
int dv_model_graph_stats(const dv_model* m, int64_t* captures, int64_t* replays);

/* Testing hook: copy activation buffer `index` (fp16, channel-blocked
 * [n][c/8][h][w][8], first n examples of the last dv_model_infer) to host
 * memory and report its (padded) shape.  index -1 = the last Inception block's
 * output (what GlobalAveragePooling reads), -2 = the stem's output. */
int dv_model_debug_tensor(dv_model* m, int index, int n, void* host_out,
                          int32_t* h, int32_t* w, int32_t* c);

/* Average time of kernels launched by the last dv_model_infer /
 * dv_encode_batch on `stream`, measured with HIP events around each launch
 * when profiling is on.  kind: 0 = encoder kernel, 1 = all conv kernels,
 * 2 = everything else.  Returns milliseconds summed over the call. */
int dv_set_profiling(int enabled);
double dv_profile_ms(int kind);
/* Number of launches summed by the last dv_profile_ms call. */
int dv_last_profile_count(void);

/* ---- postprocess_variants: the genotype merge of each site (csrc/genotype.hip) ----
 * A site is one candidate; its items are its images, contiguous: site s owns items [site_off[s], site_off[s + 1]).
 * Item i carries the classifier's probs[i][0..2] and one or two 0-based alt indices item_alts[i][0..1], the second -1
 * for a single alt.  Per item the probabilities are rounded as call_variants.round_gls_batch(p, 10) does (float32,
 * then widened); per site with more than one item and t > 0, alt a is removed when the largest min(r1 + r2, 1) over
 * its single-alt items is < t (an alt without such an item stays; were all removed, the one with the largest value
 * stays, the first on ties); the items that name no removed alt are merged by the minimum per genotype of the kept
 * alleles, in VCF order, and divided by their left-to-right sum (a site of exactly one item is neither pruned nor
 * renormalised).  `t` is dv_genotype_min_nonref_prob(qual_filter).
 * Results, bit-identical from both entry points: rounded [N][3]; pred_off [S + 1], site s owning
 * (A + 1)(A + 2) / 2 slots of `predictions` by its n_alts A, the first (A' + 1)(A' + 2) / 2 valid for its A' kept
 * alts and the rest 0; best [S], the first index of the largest prediction; removed [S], bit a set for a removed alt;
 * status [S].  DV_GENOTYPE_BAD_SUM: an item's float32 sum is off by more than 1e-6 (it outranks INCOMPLETE; the site's
 * other results are computed all the same).  DV_GENOTYPE_INCOMPLETE: a genotype of the kept alleles got no
 * contribution; its slot is +inf, the site's slots are not renormalised and best is -1.
 * Null pointers with non-zero counts or negative counts: DV_ERR_INVALID_ARGUMENT.  site_off that does not ascend from
 * 0 to n_items, n_alts outside 1..32, an alt index outside [0, A) or a second index equal to the first:
 * DV_ERR_BAD_INPUT.  On any error *out is NULL and nothing stays allocated. */
#define DV_GENOTYPE_DEVICE_MAX_ALTS 6 /* 28 genotypes; and at most 21 items, alt_allele_combinations of 6 alts */
enum { DV_GENOTYPE_OK = 0, DV_GENOTYPE_BAD_SUM = 1, DV_GENOTYPE_INCOMPLETE = 2 };
typedef struct dv_genotypes dv_genotypes; /* owns the host arrays of one call's result */
typedef struct dv_genotypes_view {        /* views into the result; valid until dv_genotypes_free */
  int32_t n_sites;
  int32_t reserved;
  int64_t n_items;
  int64_t n_predictions;
  const double* rounded;
  const int64_t* pred_off;
  const double* predictions;
  const int32_t* best;
  const uint32_t* removed;
  const uint8_t* status;
} dv_genotypes_view;
/* Host code: the twin every test compares against.  already_rounded != 0: `probs` holds the rounded values of an
 * earlier run (CallVariantsOutput records; the rounding is not idempotent) and is widened as it is; the sum is still
 * checked. */
int dv_genotype_sites(const float* probs, int64_t n_items, const int8_t* item_alts, int32_t n_sites,
                      const int32_t* site_off, const int32_t* n_alts, double t, int32_t already_rounded,
                      dv_genotypes** out);
/* The same in one launch, one lane per site; `probs` is read where it lies (probs_memory: dv_memory), the other
 * tables are host arrays.  One staged upload, one download, one synchronisation on `stream` (NULL = a non-blocking
 * stream the library owns; device-resident probs must then be complete before the call).  A site with more than
 * DV_GENOTYPE_DEVICE_MAX_ALTS alts or more than 21 items is merged by the host code inside the call and counted; a
 * call without any other site launches nothing.  No site is DV_OK without a device; no device is DV_ERR_NO_DEVICE. */
int dv_genotype_sites_device(const float* probs, int32_t probs_memory, int64_t n_items, const int8_t* item_alts,
                             int32_t n_sites, const int32_t* site_off, const int32_t* n_alts, double t,
                             dv_genotypes** out, void* stream);
int dv_genotypes_arrays(const dv_genotypes* g, dv_genotypes_view* out);
void dv_genotypes_free(dv_genotypes* g);
/* The smallest double t in [0, 1] with round(-10 * log10(1 - min(t, 1 - 1e-15)), 7) >= qual_filter (Python's round),
 * by bisection over the bit patterns: `s < t` then decides what `QUAL(s) < qual_filter` decides, without a logarithm.
 * 0 for qual_filter <= 0; +inf when no t qualifies. */
double dv_genotype_min_nonref_prob(double qual_filter);
typedef struct dv_genotype_device_stats {
  int64_t sites;         /* of the call */
  int64_t sites_on_host; /* of them above the device limit: merged by the host code */
  int64_t launches;
  int64_t bytes_down;
} dv_genotype_device_stats;
/* What the calling thread's last dv_genotype_sites_device did. */
int dv_genotype_device_last_stats(dv_genotype_device_stats* out);

/* ---- gVCF: the merge of the reference blocks with the variant records (csrc/gvcf_merge.hip) ----
 * A call carries G groups (contigs): group g owns blocks [block_off[g], block_off[g + 1]) and variants
 * [var_off[g], var_off[g + 1]), half-open spans [start, end).  Within a group the blocks are sorted and pairwise
 * disjoint, the variants sorted by (start, end); variants may overlap and nest.  A block loses what the variants
 * cover; what is left are its pieces, in order.  With the P pieces in block order and the V variants in theirs, the
 * merged sequence (merge_variants_and_nonvariants, groups in order) is a permutation of P + V slots: piece k of a group
 * comes after the group's variant j iff start[j] < piece_end[k].  P <= B + V.
 * Results, equal from both entry points: piece_start, piece_end [P]; piece_block [P], the index of the source block
 * in the call; piece_slot [P] and var_slot [V], positions in the whole call's merged sequence.
 * Null pointers with non-zero counts, a negative count or more than 2^31 - 1 records: DV_ERR_INVALID_ARGUMENT.
 * Offsets that do not ascend from 0, an empty span, blocks out of order or overlapping, variants out of (start, end)
 * order: DV_ERR_BAD_INPUT with a message.  Empty groups, and groups with blocks only or variants only, are legal.
 * On any error *out is NULL and nothing stays allocated. */
typedef struct dv_gvcf_merged dv_gvcf_merged; /* owns the host arrays of one call's result */
typedef struct dv_gvcf_merged_view {          /* views into the result; valid until dv_gvcf_merged_free */
  int64_t n_pieces;
  int64_t n_variants;
  const int64_t* piece_start;
  const int64_t* piece_end;
  const int32_t* piece_block;
  const int64_t* piece_slot;
  const int64_t* var_slot;
} dv_gvcf_merged_view;
/* Host code: the twin every test compares against. */
int dv_gvcf_merge(int32_t n_groups, const int64_t* block_off, const int64_t* var_off, const int64_t* block_start,
                  const int64_t* block_end, const int64_t* var_start, const int64_t* var_end, dv_gvcf_merged** out);
/* The same on the device; every array is a host array and is checked before any device work.  One staged upload,
 * launches queued on `stream` (NULL = a non-blocking stream the library owns), one download sized for B + V pieces,
 * one synchronisation.  A call without records is DV_OK without a device; no device is DV_ERR_NO_DEVICE. */
int dv_gvcf_merge_device(int32_t n_groups, const int64_t* block_off, const int64_t* var_off, const int64_t* block_start,
                         const int64_t* block_end, const int64_t* var_start, const int64_t* var_end,
                         dv_gvcf_merged** out, void* stream);
int dv_gvcf_merged_arrays(const dv_gvcf_merged* m, dv_gvcf_merged_view* out);
void dv_gvcf_merged_free(dv_gvcf_merged* m);
/* Elements per workgroup of the device's two scans (the running maximum of the variant ends, the sum of the piece
 * counts): a carry crosses from one workgroup's chunk to the next at multiples of it. */
int32_t dv_gvcf_merge_scan_chunk(void);
typedef struct dv_gvcf_merge_stats {
  int64_t blocks; /* of the call */
  int64_t variants;
  int64_t pieces;
  int64_t launches;
  int64_t bytes_up;
  int64_t bytes_down;
} dv_gvcf_merge_stats;
/* What the calling thread's last dv_gvcf_merge_device did. */
int dv_gvcf_merge_last_stats(dv_gvcf_merge_stats* out);

/* ---- gVCF: the rows behind the merge (csrc/gvcf_rows.hip) ----
 * The merge above, carried on to the text: every piece becomes a reference-block row (csrc/gvcf_rows.h, the format of
 * postprocess_variants._piece_rows), every variant's finished row is copied, and both stand in merged order, the
 * groups in order, without a header.  A piece that starts at its block's start prints the block's ref_base; a moved
 * start is some variant's end, and prints that variant's var_end_base.
 * Refused with DV_ERR_BAD_INPUT and a message, on the host before any device work: everything dv_gvcf_merge refuses;
 * var_text_off that does not ascend from 0; a variant row that is empty or does not end in '\n'; name_off that does
 * not ascend from >= 0; a ref_base, or a var_end_base that a piece takes, outside 0x21..0x7E; a likelihood that is
 * not finite or has |10 GL| >= 2^53.  med_dp outside -1..1 and null pointers: DV_ERR_INVALID_ARGUMENT.  Empty groups,
 * and groups with blocks only or variants only, are legal.  On any error *out is NULL and nothing stays allocated. */
typedef struct dv_gvcf_rows_input {
  int32_t n_groups;             /* G */
  int32_t med_dp;               /* the rows carry MED_DP: -1 = when any block has med_dp >= 0, else 0 or 1 */
  int32_t want_row_off;         /* also return row_off */
  int32_t reserved;
  const int64_t* block_off;     /* [G + 1] */
  const int64_t* var_off;       /* [G + 1] */
  const dv_gvcf_block* blocks;  /* [B]; start and end are the merge's block_start and block_end */
  const int64_t* var_start;     /* [V] */
  const int64_t* var_end;       /* [V] */
  const uint8_t* var_end_base;  /* [V], the reference base at var_end[j] */
  const int64_t* var_text_off;  /* [V + 1] */
  const char* var_text;         /* every variant's finished row with its '\n' */
  const int64_t* name_off;      /* [G + 1] */
  const char* names;            /* the groups' contig names, back to back */
} dv_gvcf_rows_input;
typedef struct dv_gvcf_text dv_gvcf_text;     /* owns one call's text */
typedef struct dv_gvcf_text_view {            /* views into the result; valid until dv_gvcf_text_free */
  const char* text;             /* all rows in merged order */
  int64_t n_bytes;
  const int64_t* row_off;       /* [n_rows + 1] with want_row_off, else NULL */
  int64_t n_rows;               /* n_pieces + V */
  int64_t n_pieces;
  int32_t med_dp;               /* as decided */
  int32_t reserved;
} dv_gvcf_text_view;
/* Host code: one pass per group. */
int dv_gvcf_rows(const dv_gvcf_rows_input* in, dv_gvcf_text** out);
/* The same on the device; every array is a host array.  One staged upload, launches queued on `stream` (NULL = a
 * non-blocking stream the library owns), a wait for the 16-byte header, then a download of exactly n_bytes (and
 * row_off when asked for) and a second wait.  A call without records is DV_OK without a device and launches nothing;
 * no device is DV_ERR_NO_DEVICE. */
int dv_gvcf_rows_device(const dv_gvcf_rows_input* in, dv_gvcf_text** out, void* stream);
int dv_gvcf_text_arrays(const dv_gvcf_text* t, dv_gvcf_text_view* out);
void dv_gvcf_text_free(dv_gvcf_text* t);
typedef struct dv_gvcf_rows_stats {
  int64_t blocks; /* of the call */
  int64_t variants;
  int64_t pieces;
  int64_t rows;
  int64_t text_bytes;
  int64_t launches;
  int64_t bytes_up;
  int64_t bytes_down;
} dv_gvcf_rows_stats;
/* What the calling thread's last dv_gvcf_rows_device did. */
int dv_gvcf_rows_last_stats(dv_gvcf_rows_stats* out);

/* ---- BGZF: a text deflated into members of at most 64 KiB (csrc/bgzf.hip) ----
 * The text is cut every `block` bytes; every block becomes one BGZF member (one deflate block: fixed Huffman over the
 * tokens of csrc/bgzf_deflate.h, or stored when that is shorter), and the 28-byte end-of-file member follows.  An
 * empty text gives the end-of-file member alone.  The host code and the device write the same bytes.
 * Null pointers, a negative n and an unknown `memory` are DV_ERR_INVALID_ARGUMENT; on any error *out is NULL. */
typedef struct dv_bgzf_parameters {
  int32_t block;                /* input bytes per member */
  int32_t tile;                 /* positions that read their candidates before any of them is entered */
  int32_t seg;                  /* bytes parsed greedily from their own start */
  int32_t hash_bits;
} dv_bgzf_parameters;
int dv_bgzf_params(dv_bgzf_parameters* out);
typedef struct dv_bgzf_file dv_bgzf_file;     /* owns one call's file */
typedef struct dv_bgzf_view {                 /* views into the result; valid until dv_bgzf_free */
  const uint8_t* data;          /* the members, then the end-of-file member */
  int64_t n_bytes;
  int64_t n_blocks;             /* the members with text */
  const int64_t* block_coff;    /* [n_blocks + 1]: every member's offset in the file, the end-of-file member's last */
  int64_t stored_blocks;        /* the members whose block is stored */
} dv_bgzf_view;
/* Host code; the blocks are spread over host threads. */
int dv_bgzf_compress(const void* text, int64_t n, dv_bgzf_file** out);
/* The same on the device; `text` is read where it lies (memory: dv_memory).  One staged upload (the text too when it
 * is a host array), five launches queued on `stream` (NULL = a non-blocking stream the library owns), a wait for the
 * 16-byte header, then a download of exactly n_bytes and block_coff and a second wait.  An empty text is DV_OK
 * without a device and launches nothing; no device is DV_ERR_NO_DEVICE. */
int dv_bgzf_compress_device(const void* text, int32_t memory, int64_t n, dv_bgzf_file** out, void* stream);
int dv_bgzf_arrays(const dv_bgzf_file* f, dv_bgzf_view* out);
void dv_bgzf_free(dv_bgzf_file* f);
typedef struct dv_bgzf_stats {
  int64_t text_bytes;
  int64_t file_bytes;
  int64_t blocks;
  int64_t stored_blocks;
  int64_t launches;
  int64_t bytes_up;             /* the CRC tables, and the text when it was a host array */
  int64_t bytes_down;           /* 16 + the file + block_coff */
} dv_bgzf_stats;
/* What the calling thread's last device compression did (dv_bgzf_compress_device, or the one inside
 * dv_gvcf_rows_bgzf_device). */
int dv_bgzf_last_stats(dv_bgzf_stats* out);

/* dv_gvcf_rows[_device] with `prefix` (the header, n_prefix bytes) in front, compressed instead of returned: *file is
 * the BGZF file of prefix + rows, *meta says what the text was.  in->med_dp must be 0 or 1 here, since the header that
 * names MED_DP is written before the call.  Refused: everything dv_gvcf_rows refuses, a negative n_prefix, med_dp -1.
 * On the device the text is never downloaded: the rows are written behind the prefix in device memory and deflated
 * there; dv_gvcf_rows_last_stats then counts the rows' launches and bytes, dv_bgzf_last_stats the compressor's. */
typedef struct dv_gvcf_rows_meta {
  int64_t n_rows;
  int64_t n_pieces;
  int64_t text_bytes;           /* n_prefix + the rows */
  const int64_t* row_off;       /* [n_rows + 1] into prefix + rows with want_row_off, else NULL; freed with *file */
} dv_gvcf_rows_meta;
int dv_gvcf_rows_bgzf(const dv_gvcf_rows_input* in, const void* prefix, int64_t n_prefix, dv_gvcf_rows_meta* meta,
                      dv_bgzf_file** file);
int dv_gvcf_rows_bgzf_device(const dv_gvcf_rows_input* in, const void* prefix, int64_t n_prefix, dv_gvcf_rows_meta* meta,
                             dv_bgzf_file** file, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DVHIP_H_ */
