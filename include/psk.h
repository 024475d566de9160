/*
 * psk.h -- C ABI of libpsk.so, the MI355X (gfx950) k-mer association engine that replaces the
 * hot path of bioinfo-ut/PhenotypeSeeker's `modeling` / `prediction` commands.
 *
 * Plain C: opaque context, caller-owned host buffers in and out, sizes as integers, every
 * function returns 0 on success or a negative PSK_E* code (psk_last_error() has the text).
 * No torch types, no C++ types.  One context drives one GPU from one host thread; create one
 * context per rank for multi-GPU runs (the k-mer word space is range-sharded, see psk_begin).
 *
 * Each entry point cites the reference interface it replaces (paths under /root/reference;
 * modeling.py = PhenotypeSeeker/modeling.py, prediction.py = PhenotypeSeeker/prediction.py).
 * The reference's own boundary for this path is a set of subprocess command lines plus Python
 * methods; INTEGRATION.md shows the ctypes stubs that rebind those call sites to this ABI.
 */
#ifndef PSK_H
#define PSK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct psk_ctx psk_ctx;

enum {
    PSK_OK = 0,
    PSK_EINVAL = -1,   /* bad argument / call order */
    PSK_ENOMEM = -2,   /* host or device allocation failed */
    PSK_EHIP = -3,     /* a HIP runtime call failed */
    PSK_ERANGE = -4,   /* caller buffer too small / size limit exceeded */
    PSK_ESTATE = -5,   /* required earlier stage has not been run */
    PSK_EGZIP = -6     /* (with PSK_NO_GPU_GZ=1 only; r05: .gz inputs are inflated by the library) a FILE input is gzip-compressed
                          (magic bytes): the caller inflates it and uses the in-memory call */
};

/* ---- lifecycle --------------------------------------------------------------------------- */

/* Binds a context to HIP device `device` (creates its stream and timing events). */
int psk_init(int device, psk_ctx **ctx_out);
void psk_free(psk_ctx *ctx);
/* Text of the last error on this context (or of the failed psk_init when ctx is NULL). */
const char *psk_last_error(const psk_ctx *ctx);
/* ABI version of the library: (major << 16) | minor. */
int psk_version(void);
/* Device facts for reports: name (NUL-terminated, truncated to name_cap), CU count, HBM bytes. */
int psk_device_info(psk_ctx *ctx, char *name, int name_cap, int *n_cu, uint64_t *hbm_bytes);

/*
 * Starts a k-mer run: word length k (1..32; modeling.py:161 `-l`), the number of samples that
 * will be counted, and this context's shard [slab_lo, slab_hi) of the canonical 2k-bit word
 * space (slab_hi == 0 means "to the end"; one GPU: 0, 0).  Drops all state of a previous run.
 */
int psk_begin(psk_ctx *ctx, int k, int n_samples, uint64_t slab_lo, uint64_t slab_hi);

/* ---- a1: per-sample k-mer list ------------------------------------------------------------
 * Replaces `glistmaker <addr> -o K-mer_lists/<name>_0 -w <k> -c <cutoff>`
 * (Samples.get_kmer_lists, modeling.py:303-315; bundled binary bin/glistmaker 4.2.3).
 * `bytes` is the inflated FASTA/FASTQ file image.  The sorted canonical list (words + u32
 * frequencies, exactly the records of glistmaker's .list file, restricted to the slab) stays
 * in HBM under `sample_idx`; n_unique / n_total report its size.  As in the bundled binary,
 * no frequency cut-off is applied.
 */
int psk_count_kmers(psk_ctx *ctx, int sample_idx, const uint8_t *bytes, size_t len, uint64_t *n_unique,
                    uint64_t *n_total);
/* Batch form of psk_count_kmers for samples first_sample_idx .. first_sample_idx + n - 1: n_threads host
 * threads tokenise ahead into a ring of pinned buffers while the calling thread drives the GPU half
 * in order, so host framing overlaps device work.  n_unique / n_total: n entries each (may be NULL). */
int psk_count_kmers_batch(psk_ctx *ctx, int first_sample_idx, int n, const uint8_t *const *bytes, const size_t *lens,
                          uint64_t *n_unique, uint64_t *n_total, int n_threads);
/* The same call that also returns every sample's MinHash sketch (psk_minhash_sketch below) from the clean
 * stream that is already on the device for counting: the `-w` path (get_kmer_lists + get_mash_sketches,
 * modeling.py:303-315, :386-390) needs both and each file is framed and uploaded once.
 *   sketch_k == 0: no sketches (hashes_out / n_hashes_out may be NULL)
 *   hashes_out[n][sketch_size] ascending distinct hashes, n_hashes_out[n] = how many of each row are valid
 */
int psk_count_kmers_batch_sketch(psk_ctx *ctx, int first_sample_idx, int n, const uint8_t *const *bytes,
                                 const size_t *lens, uint64_t *n_unique, uint64_t *n_total, int n_threads,
                                 int sketch_k, int sketch_size, uint32_t sketch_seed, uint64_t *hashes_out,
                                 uint64_t *n_hashes_out);
/* The same for UNCOMPRESSED files on disk (paths[i] of sizes[i] bytes): the framing threads read them, so no file
 * image crosses the caller's language boundary.  A .gz file is read as it is and inflated by the library (psk_gz_inflate
 * below says how). */
int psk_count_kmers_files(psk_ctx *ctx, int first_sample_idx, int n, const char *const *paths, const size_t *sizes,
                          uint64_t *n_unique, uint64_t *n_total, int n_threads, int sketch_k, int sketch_size,
                          uint32_t sketch_seed, uint64_t *hashes_out, uint64_t *n_hashes_out);
/* .gz inputs ("FASTA/FASTQ(.gz)", glistmaker's zlib reader: SURVEY.md section 2 row 9).  psk_count_kmers /
 * psk_count_kmers_batch / psk_count_kmers_files take a gzip image (magic bytes 1f 8b) as it is: the compressed bytes
 * cross PCIe and DEFLATE is decoded on the device (csrc/gz_inflate.hip) -- all .gz samples of a call together, 8 GiB of text
 * at a time (PSK_GZ_GROUP_MB); a group of so few small files that zlib would be faster (the device route has a floor of ~40 ms) and a member the device
 * route declines go through zlib on the call's host threads.  This entry point is the inflate on its own -- tests and measurements: n gzip images ->
 * their text (out[i], of capacity out_cap[i], may be NULL: lengths only).  route[i]: 1 decoded on the device, 2 the same,
 * a BGZF file (its members found by their BSIZE fields), 0 zlib on the host, -1 zlib refused the file.  A refused file fails
 * the call (PSK_EINVAL, zlib's words for the first one, as glistmaker's reader fails) -- after every file has been tried: with
 * `route` given, the texts and lengths of the other files are delivered all the same.  device_ms: wall-clock of the device
 * route, upload included.  PSK_GZ_GUARD=1 (the fuzz test): 64-KB guard bands around the device buffers, checked after the
 * last kernel (PSK_ESTATE when one was written to). */
int psk_gz_inflate(psk_ctx *ctx, int n, const uint8_t *const *data, const size_t *sizes, uint8_t *const *out,
                   const size_t *out_cap, uint64_t *out_len, int32_t *route, double *device_ms);
/* Copies sample_idx's list to the host (for writing .list files / parity checks). */
int psk_get_list(psk_ctx *ctx, int sample_idx, uint64_t *words, uint32_t *freqs, uint64_t cap);
/* ---- multi-GPU ingest: count each sample on ONE rank, exchange the slab ranges of the sorted lists ----------
 * (no counterpart in the reference, which has no multi-process counting; see phenotypeseeker_amd/dist.py
 * ListExchange.)  A slab of the word space is a contiguous range of a sorted list, so the hand-over is three calls:
 *   psk_lists_split     offsets_out[i * n_bounds + b] = number of words of sample first + i below bounds[b]
 *                       (bounds ascending; a bound of 0 after the first entry means "end of the word space")
 *   psk_copy_list_ranges  packs ranges [start[r], start[r] + count[r]) of the lists sample_idx[r], back to back,
 *                         into DEVICE buffers (the send buffers of the all-to-all); waited for
 *   psk_set_lists_device  installs n_lists lists held back to back in DEVICE memory -- count[r] (word, count)
 *                         entries each, ascending, inside this context's slab (checked: PSK_EINVAL otherwise, and
 *                         none of them is kept) -- as the lists of sample_idx[r]; they are copied into the
 *                         context's own storage.  n_total[r] (may be NULL) is what psk_count_kmers would report.
 *   psk_release_lists   gives the device memory of this context's lists back (every sample is "not counted"
 *                       again): the counting context's lists are dead once they are packed, and at N = 2 of
 *                       config 3 they are 61 GB that the receive buffers need */
int psk_lists_split(psk_ctx *ctx, int first_sample_idx, int n, const uint64_t *bounds, int n_bounds,
                    uint64_t *offsets_out);
int psk_copy_list_ranges(psk_ctx *ctx, int n_ranges, const int32_t *sample_idx, const uint64_t *start,
                         const uint64_t *count, void *device_words_dst, void *device_freqs_dst);
int psk_release_lists(psk_ctx *ctx);
int psk_set_lists_device(psk_ctx *ctx, int n_lists, const int32_t *sample_idx, const uint64_t *count,
                         const uint64_t *n_total, const void *device_words, const void *device_freqs);
/* Frequencies of `n` given canonical words in sample_idx's list (0 if absent): the
 * `glistquery <sample>.list -l` mapping of modeling.py:324-329 restricted to the k-mers the
 * caller still needs (--real_counts columns of the ML matrix, modeling.py:693-695). */
int psk_lookup_counts(psk_ctx *ctx, int sample_idx, const uint64_t *words, uint64_t n, uint32_t *freqs);

/* ---- a2+a3: feature vector (union) and the k-mer x sample presence matrix ------------------
 * Replaces the `glistcompare -u` reduction tree (Samples.get_feature_vector / get_union,
 * modeling.py:350-380) and the per-sample `glistquery ... -l feature_vector.list` + `split`
 * text mapping (Samples.map_samples, modeling.py:317-348).  Result, resident in HBM:
 *   words[M]            ascending canonical words of the union (this slab)
 *   bits[M][wpr]        u64 words, sample i = bit (i & 63) of word (i >> 6); wpr = 1 up to 64 samples, else even
 * n_kmers = M is this slab's share of phenotypes.no_kmers_to_analyse (modeling.py:644).
 */
int psk_build_presence(psk_ctx *ctx, uint64_t *n_kmers);
int psk_presence_shape(psk_ctx *ctx, uint64_t *n_kmers, int *words_per_row, int *n_samples);
int psk_get_union(psk_ctx *ctx, uint64_t *words, uint64_t cap);
/* Gathers `n` rows (by row index) of the matrix: bits_out[n][words_per_row]. */
int psk_get_rows(psk_ctx *ctx, const uint64_t *row_idx, uint64_t n, uint64_t *bits_out);
/* a9, phenotypes.get_ML_df (modeling.py:1112-1145, rows built at :739 / :796): writes `path` = <test>_results_<pheno>.tsv --
 * `header`, then one line per k-mer that passed the scan: k-mer, round(stat, 2), "%.2E" % p, [round(mean_x, 2),
 * round(mean_y, 2) when kind = 1 (t-test),] n_with, "| " + the names of the VALID samples (valid[i] != 0: phenotype not NA)
 * whose bit is set in the k-mer's row -- and, when path_top is not NULL, its first n_top lines again as `path_top`
 * (:1133-1136).  Lines are ordered by the p-value STRINGS as the reference orders them (:1128), ties by k-mer;
 * order_out[n_rows] receives that order (row indices).  words[n_rows] 2-bit words of length k; bits[n_rows][wpr] as
 * psk_get_rows returns them; names = the sample names back to back, name i = bytes [name_off[i], name_off[i + 1]).
 * Host code (no GPU work; ctx may be NULL: it only carries the error text).  Every byte equals what the reference's
 * DataFrame.to_csv wrote for the same rows: floats as Python's repr, tests/golden/ds_* hold the files. */
int psk_write_result_tables(psk_ctx *ctx, const char *path, const char *path_top, int64_t n_top, const char *header, int kind,
                            int64_t n_rows, const uint64_t *words, int k, const double *stat, const double *p,
                            const double *mean_x, const double *mean_y, const int32_t *n_with, const uint64_t *bits,
                            int words_per_row, int n_samples, const uint8_t *valid, const char *names, const int64_t *name_off,
                            int64_t *order_out);
/* a11, write_model_coefficients_to_file (modeling.py:1414-1455): APPENDS to `path` (whose header line the caller has written)
 * one line per k-mer of the model: k-mer \t repr(coefficient) \t number of samples with it \t "| " + their names.  kmers /
 * kmer_off and names / name_off: texts back to back with their offsets; x[n_samples][n_kmers] (int64, row-major): the model
 * matrix of <pheno>_MLdf.csv, a sample carries a k-mer where it is not 0.  Host code; ctx may be NULL. */
int psk_write_model_coefficients(psk_ctx *ctx, const char *path, int64_t n_kmers, const char *kmers, const int64_t *kmer_off,
                                 const double *coefs, const int64_t *x, int64_t n_samples, const char *names,
                                 const int64_t *name_off);
/* `--kmerDB`: keeps only rows whose word occurs in the (sorted, canonical) db word list --
 * `glistcompare -i` of Samples.get_db_kmers, modeling.py:367-372. */
int psk_intersect_db(psk_ctx *ctx, const uint64_t *db_words, uint64_t n_db, uint64_t *n_kmers);
/* Loads an externally built matrix instead (tests, benchmarks): words may be NULL. */
int psk_set_presence(psk_ctx *ctx, const uint64_t *words, const uint64_t *bits, uint64_t n_kmers,
                     int words_per_row, int n_samples);
/* Fills the resident matrix with a synthetic pattern on the device (benchmark only):
 * row r is present in sample i with a probability that depends on r; see DESIGN.md.  Bits 48..63 of `seed`, when not
 * zero, thin the 1 % of "gene" rows (the rows that survive a scan against the even/odd phenotype) to that many in 10,000
 * of them: 80 gives BASELINE config 2's survivor share. */
int psk_synth_presence(psk_ctx *ctx, uint64_t n_kmers, int n_samples, uint64_t seed);

/* ---- a4-a6: chi-squared scan ---------------------------------------------------------------
 * Replaces phenotypes.get_kmers_tested + conduct_chi_squared_test and helpers
 * (modeling.py:677-714, :759-858) for one binary phenotype.
 *   pheno[n_samples]    1, 0, or -1 for 'NA' (modeling.py:122-126, :810/:817)
 *   weights[n_samples]  GSC weights, or NULL for unit weights (modeling.py:284,:812-822)
 *   min/max_samples     Samples.min_samples / max_samples (modeling.py:233-242,:770-772)
 *   pvalue_cutoff, omit_B, n_kmers_global   the filter of modeling.py:795; n_kmers_global is
 *                       the Bonferroni denominator = union size summed over all slabs
 * Surviving rows are kept on the device; fetch them with psk_get_results.
 */
int psk_chi2_scan(psk_ctx *ctx, const int8_t *pheno, const double *weights, int min_samples, int max_samples,
                  double pvalue_cutoff, int omit_B, uint64_t n_kmers_global, uint64_t *n_pass);
/* The same scan in two halves: _begin launches it and returns, psk_scan_end waits for the OLDEST scan in flight and
 * yields its number of surviving k-mers (with none in flight: the last count again).  Up to two scans may be in
 * flight -- there are two result sets -- so the multi-GPU step runs begin(i+1), end(i), export(i), begin(i+2),
 * all-gather(i): the device always has the next scan queued while the host handles the previous one's survivors.
 * The result calls (psk_get_results, psk_export_survivors*) read the last scan ENDED.  A psk_chi2_scan_begin issued
 * with no scan in flight takes the OTHER result set, so the next scan can be launched before the last one's results
 * are read (the pipeline over phenotypes: end(j), begin(j+1), read j); issued while a scan is in flight it takes
 * the set of the last scan ended (after any asynchronous export of it, on the device), and the result calls fail
 * with PSK_ESTATE until the next psk_scan_end.  A third _begin, and the one-call scans while a scan is in flight,
 * fail with PSK_ESTATE.
 * What "ended" means.  The scan's survivor count is final and every call of this library that reads its results --
 * psk_get_results, psk_export_survivors, psk_export_survivors_async on any stream, the next scans -- sees all of
 * them: each is ordered behind the scan on the device.  It does NOT mean that the scan's dispatch has retired: an
 * unweighted scan is ended by the words its kernel writes to pinned memory (PSK_SCAN_WAIT, docs/KNOBS.md), which
 * arrive as its last workgroups finish.  Of a launch of at most 64 workgroups (the index form of the side-matrix scan)
 * psk_scan_end reads one summary line -- n_pass, the scan's end clock, an overflow flag -- written by the last
 * workgroup to publish a segment (PSK_SCAN_SUMMARY; a larger launch is waited for segment by segment); the per-segment
 * counts are read, and checked to be this scan's and to add up to n_pass, by the first result call made on the scan,
 * which may therefore be the call that reports PSK_ESTATE for a scan whose words never arrived.  PSK_ERANGE (a segment
 * overflowed) still comes from psk_scan_end: the summary says so.  A scan whose set is taken by a later
 * psk_chi2_scan_begin before any result call never has its counts read.  A caller that reads the context's device buffers by means of its own, on a
 * stream of its own, synchronises with the context first (any blocking call of this library does).  Once
 * psk_export_survivors_async has been called on a context its scans are ended by events again (the dispatch has
 * completed when psk_scan_end returns), so the export never waits for a later scan already queued. */
int psk_chi2_scan_begin(psk_ctx *ctx, const int8_t *pheno, const double *weights, int min_samples, int max_samples,
                        double pvalue_cutoff, int omit_B, uint64_t n_kmers_global);
int psk_scan_end(psk_ctx *ctx, uint64_t *n_pass);

/* ---- a7: weighted Welch t-test scan ---------------------------------------------------------
 * Replaces conduct_t_test + get_samples_distribution_for_ttest (modeling.py:716-757) for one
 * continuous phenotype; valid[i] == 0 marks 'NA'.  Bonferroni is always applied (:738).
 */
int psk_ttest_scan(psk_ctx *ctx, const double *pheno, const uint8_t *valid, const double *weights,
                   int min_samples, int max_samples, double pvalue_cutoff, uint64_t n_kmers_global,
                   uint64_t *n_pass);

/* Results of the last scan, ascending by row index (= ascending k-mer).  Any pointer may be
 * NULL.  stat = chi2 or t; mean_x / mean_y are filled by the t-test only. */
int psk_get_results(psk_ctx *ctx, uint64_t *row_idx, uint64_t *words, double *stat, double *p, double *mean_x,
                    double *mean_y, int32_t *n_with, uint64_t cap);
/* Multi-GPU hand-off: writes the survivors of the last scan, unsorted, as records of (6 + words_per_row)
 * u64 { word, stat, p, mean_x, mean_y (f64 bit patterns), n_with (i64), bits[words_per_row] } into a
 * caller-provided DEVICE buffer of 1 + cap_records records; record 0 is a header whose first u64 is the
 * record count.  The buffer can be handed to an RCCL all-gather as is (phenotypeseeker_amd/dist.py).
 * n_records returns the count; records beyond cap_records are dropped (caller retries with a larger cap). */
int psk_export_survivors(psk_ctx *ctx, void *device_dst, uint64_t cap_records, uint64_t *n_records);
/* The same export queued on the CALLER's stream (a hipStream_t, e.g. torch's current stream) and not waited for:
 * work queued on that stream afterwards -- the RCCL all-gather -- is ordered behind it without a host
 * synchronisation; the next scan that writes the same result set waits on the device for the export to finish.
 * The export itself is ordered behind the scan it reads, on the device, whichever way that scan was ended. */
int psk_export_survivors_async(psk_ctx *ctx, void *device_dst, uint64_t cap_records, void *stream);
/* Whether the current matrix has an exception-coded copy for the unweighted chi2 scan (*encoded = 1; 65..256 samples,
 * rows mostly within 7 samples of all-absent or all-present), and how many of its rows sit in the side matrix of dense
 * rows (*overflow_rows).  Measurement and tests only: the scan picks its form by itself (PSK_SCAN_DENSE=1 forces the dense one). */
int psk_compact_info(const psk_ctx *ctx, int *encoded, uint64_t *overflow_rows);
/* 1 when the division-free pre-test of the unit-weight chi2 scan lets the 2 x 2 table (A, B | C, D) through to the exact
 * evaluation against the statistic threshold thr = -2 log(cut), else 0: the host's evaluation of the function the dense
 * kernel and the exception-coded scan's candidate table share.  Tests only (no context, no device). */
int psk_chi2_pretest(double A, double B, double C, double D, double thr);
/* What the exception-coded scan makes of a scan's parameters (class sizes n1, n0 of n_samples samples, the frequency
 * filter, the statistic threshold thr of the pre-test) before it launches.  corner[base] bit a' * 8 + c' (a', c' <= 7):
 * a row with a' case and c' control exceptions -- its table is (a', c') when the exceptions are the present samples
 * (base 0), (n1 - a', n0 - c') when they are the absent ones (base 1) -- passes the frequency filter and the pre-test;
 * 0 where a' > n1 or c' > n0.  *class_mask bit (e | base << 3): a row of e = 0..7 exceptions can have such a table; its
 * exceptions among the n_samples - n1 - n0 NA samples count towards neither a' nor c'.  A class whose bit is clear is
 * dropped on its header byte; with no bit set the scan does not read the slots at all.  Host code: no context, no device. */
int psk_cx_plan(int n1, int n0, int n_samples, int min_samples, int max_samples, double thr, uint32_t *class_mask,
                uint64_t *corner /* [2] */);
/* The launch shape of the side-matrix kernel (chi2_scan_kernel_cx_side) of a scan with no feasible slot class: n_ov
 * overflow rows of cpr (1 or 2) 16-byte chunks, at most cap_blocks workgroups.  *blocks = workgroups of the launch (what
 * one batch per wave needs, capped, never below the 256 result segments); a wave takes the batches of *batch_rows rows
 * w, w + W, ... of the W = 4 * blocks waves; *rows_per_block bounds the rows one workgroup visits (it sizes the result
 * segments).  batch_rows may be NULL.  Host code: no context, no device. */
int psk_cx_side_shape(uint64_t n_ov, int cpr, uint64_t cap_blocks, uint32_t *blocks, uint64_t *rows_per_block,
                      uint32_t *batch_rows);
/* What a chi2 scan's parameters leave of the side matrix, by popcount: bit pc (0 ... 255) of feas[4] is set exactly when a
 * row with pc of the n_samples valid samples present can have a 2 x 2 table that passes the frequency filter and
 * psk_chi2_pretest -- its a + c lies in [max(0, pc - n_na), min(pc, n1 + n0)], n_na = n_samples - n1 - n0, and for each
 * sum the two tables at the ends of a's range decide.  n_samples <= 256.  Host code: no context, no device. */
int psk_cx_pc_plan(int n1, int n0, int n_samples, int min_samples, int max_samples, double thr, uint64_t *feas /* [4] */);
/* The launch shape of the popcount-filtered side-matrix kernel (chi2_scan_kernel_cx_side_pc): as psk_cx_side_shape, with
 * one row per lane -- *batch_rows = 64 x the kernel's unroll, whatever the row's width. */
int psk_cx_pc_shape(uint64_t n_ov, uint64_t cap_blocks, uint32_t *blocks, uint64_t *rows_per_block, uint32_t *batch_rows);
/* The side-matrix filter of the last chi2 scan launched or repeated on the context: *filtered = 1 when it ran the
 * popcount-filtered kernel (a side-kernel plan, PSK_CX_PC_FILTER not 0, fewer feasible rows than overflow rows),
 * *rows_feasible = the overflow rows whose popcount psk_cx_pc_plan leaves (all of them when the plan was not asked:
 * no side-kernel plan, or the knob off), *rows_overflow = the rows of the side matrix; all 0 for a scan that did not
 * take the exception-coded path.  Measurement and tests only.  Any pointer may be NULL. */
int psk_last_scan_filter(const psk_ctx *ctx, int *filtered, uint64_t *rows_feasible, uint64_t *rows_overflow);
/* The kernel form of the last chi2 scan set up on the context: 0 dense, 1 the mixed exception-coded kernel, 2 the side
 * matrix alone, 3 the side matrix through its popcounts, 4 the feasible rows of the side matrix through the index by
 * popcount (forms 3 and 4 are both "filtered" to psk_last_scan_filter); -1 before any.  Measurement and tests only. */
int psk_last_scan_form(const psk_ctx *ctx, int *form);
/* Where a scan's feasible rows lie in the encoder's index of the side matrix by popcount (rows grouped by popcount, bucket
 * pc starting at the exclusive prefix of pc_hist[0 .. n_hist)): the feasible (bit pc of feas[4]), non-empty buckets as
 * ranges [begin[i], begin[i] + len[i]) of index positions, buckets that follow each other in the index merged.  *n_runs =
 * all ranges there are, of which the first 4 are written (the rest of begin / len: 0); *rows = the rows in all of them;
 * *chosen = 1 when a filtered scan of a side matrix of n_ov rows would run the index form: knob_on (PSK_CX_PC_INDEX),
 * at most 4 ranges and rows x 8 <= n_ov.  rows and chosen may be NULL.  Host code: no context, no device. */
int psk_cx_idx_plan(const uint64_t *feas /* [4] */, const uint64_t *pc_hist, int n_hist, uint64_t n_ov, int knob_on,
                    uint64_t *begin /* [4] */, uint64_t *len /* [4] */, int *n_runs, uint64_t *rows, int *chosen);
/* The launch shape of the index form (chi2_scan_kernel_cx_side_idx) for n_rows feasible rows: *blocks = what one row per
 * thread needs, at least 1, at most cap_blocks -- NOT raised to the 256 result segments; workgroup b visits rows
 * (p * blocks + b) * threads + thread in pass p; *rows_per_block = passes x *threads; *seg_cap = the entries of a result
 * segment that follow.  threads and seg_cap may be NULL.  Host code: no context, no device. */
int psk_cx_idx_shape(uint64_t n_rows, uint64_t cap_blocks, uint32_t *blocks, uint64_t *rows_per_block, uint32_t *threads,
                     uint64_t *seg_cap);
/* Debug read-back of the encoder's index (tests): the positions of the side-matrix rows grouped by popcount into
 * index[0 .. cap) (cap >= the overflow rows of psk_compact_info; PSK_ERANGE otherwise) and the buckets' starts, the
 * exclusive prefix of the popcount histogram, into pc_start[0 .. n_start), n_start <= n_samples + 2.  PSK_ESTATE when
 * the matrix has no exception-coded copy.  Either pointer may be NULL. */
int psk_cx_pc_index(psk_ctx *ctx, uint32_t *index, uint64_t cap, uint64_t *pc_start, int n_start);
/* The plan of the last chi2 scan launched or repeated on the context: *encoded = 1 when it took the exception-coded path
 * (else the other two are 0), *class_mask as psk_cx_plan gives it, *slots_skipped = 1 when the launch read only the side
 * matrix of overflow rows.  Measurement and tests only.  Any pointer may be NULL. */
int psk_last_scan_plan(const psk_ctx *ctx, int *encoded, uint32_t *class_mask, int *slots_skipped);
/* Duration of the last scan in milliseconds (for bench.py): from the start and end clock words its kernel stamped (an
 * unweighted chi2 scan ended by psk_scan_end: its first instruction to the publish of its last segment; PSK_SCAN_WAIT=0:
 * its event pair), else the HIP-event duration of its kernel launches. */
double psk_last_scan_ms(const psk_ctx *ctx);
/* Re-launches the last chi2 scan `reps` times back to back on the context's stream and
 * returns the mean kernel duration in ms measured with HIP events on that stream. */
int psk_rescan_timed(psk_ctx *ctx, int reps, double *mean_ms);
/* The same, returning the HIP-event duration of every one of the `reps` launches in ms_each[reps] (bench.py: the
 * min / median / 95th percentile of the headline kernel; measurement only, no reference call site). */
int psk_rescan_times(psk_ctx *ctx, int reps, double *ms_each);

/* Measurement only (the scan's achieved bandwidth is quoted "against both the 8 TB/s spec and
 * the measured stream-read ceiling"; no reference call site -- the reference has no notion of bandwidth): reads the
 * presence matrix of the context once per launch with a kernel that does nothing else (16 B per lane), `reps` launches
 * timed with HIP events on the context's stream.  Four shapes of that kernel are timed (grid-stride or the scan's own
 * wave-contiguous pieces, non-temporal or plain loads): the fastest is the ceiling, *shape (0..3) says which.
 * *bytes_per_launch = rows x 8 x words per row as stored. */
int psk_stream_read_ceiling(psk_ctx *ctx, int reps, double *mean_ms, uint64_t *bytes_per_launch, int *shape);

/* ---- a10: L1 models over the selected k-mers ------------------------------------------------
 * Replaces the estimator fits behind GridSearchCV (modeling.py:994-1014, :1075-1085,
 * :1208-1216): every (grid value, fold) pair and the refits are independent problems and are
 * solved one per workgroup.
 *   X[n][p]      row-major float design matrix (presence 0/1, or counts with --real_counts)
 *   fold[n]      test-fold id of each sample in 0..n_folds-1; a fit with fold id f trains on
 *                samples whose fold != f; fit_fold[j] == -1 trains on all samples
 *   fit_param[j] C (logistic) or alpha (lasso) of fit j;  n_fits fits in total
 *   coef_out[n_fits][p], icpt_out[n_fits]
 * Logistic: liblinear's L1R_LR objective ||w||_1 + |b| + C sum log(1+exp(-y(w.x+b))).
 * Lasso: (1/2n)||y - Xw - b||^2 + alpha ||w||_1, unpenalised intercept.
 * Device scratch for the duration of the call: the design in both orientations and the per-fit state (a few MB); a 0/1
 * design of up to 4096 samples with 193..1024 columns (65..1024 from 1,024 samples on) also takes a per-fit Gram matrix, n_fits x ~4 p^2 bytes
 * (0.5 GB for 143 fits of 907 columns; the form is skipped beyond 32 GB).
 */
int psk_logreg_l1_fit(psk_ctx *ctx, const float *X, const int32_t *y01, int n, int p, const int32_t *fold,
                      const double *fit_param, const int32_t *fit_fold, int n_fits, double tol, int max_iter,
                      double *coef_out, double *icpt_out, int32_t *iters_out);
int psk_lasso_fit(psk_ctx *ctx, const float *X, const double *y, int n, int p, const int32_t *fold,
                  const double *fit_param, const int32_t *fit_fold, int n_fits, double tol, int max_iter,
                  double *coef_out, double *icpt_out, int32_t *iters_out);

/* ---- f17: L1 logistic regression with a free intercept (`--penalty L1 --logreg_solver saga`) --------
 * Replaces GridSearchCV over LogisticRegression(penalty='l1', solver='saga') (set_model, modeling.py:1011-1014,
 * get_logreg_solver :245-264).  Same batching, argument meaning, routes, placements and form knobs as
 * psk_logreg_l1_fit; the objective is the one saga minimises,
 *   ||w||_1 + C sum log(1+exp(-y(w.x+b))),   the intercept b unpenalised,
 * and the contract is its optimum reached to liblinear's stopping rule at the caller's tolerance (saga's own
 * stochastic iterate is no target: it stops at its iteration limit above the optimum, or after a few epochs):
 * ||violation||_1 <= tol min(#pos, #neg) / l x ||violation at w = 0, b = 0||_1, the intercept's violation being
 * |d/db|.  Same scheme as psk_logreg_l1_fit (outer Newton steps, inner coordinate descent with shrinking, one
 * Armijo line search); the intercept is never shrunk, stepped by -G / H without a soft threshold and left out of
 * the line search's ||w||_1.  iters_out = Newton steps.  A fit whose training samples are of one class has no
 * minimiser (b runs off to infinity) and is refused (PSK_EINVAL, naming the fit). */
int psk_logreg_l1_free_fit(psk_ctx *ctx, const float *X, const int32_t *y01, int n, int p, const int32_t *fold,
                           const double *fit_param, const int32_t *fit_fold, int n_fits, double tol, int max_iter,
                           double *coef_out, double *icpt_out, int32_t *iters_out);

/* ---- f4: the `--penalty L2` estimators --------------------------------------------------------
 * Replaces GridSearchCV over Ridge (set_model, modeling.py:1001-1002) and over
 * LogisticRegression(penalty='l2', solver=<-ls>) (modeling.py:1015-1019, get_logreg_solver :256-264).
 * Same batching and argument meaning as the L1 fits above.
 * Ridge: ||y - Xw - b||^2 + alpha ||w||^2 over the training rows, unpenalised intercept (sklearn's
 *   fit_intercept centring); solved to convergence (scikit-learn's dense solve is direct), so there is
 *   no tol / max_iter.  iters_out = conjugate-gradient steps.
 * Logistic: 0.5 (w'w [+ b^2]) + C sum log(1+exp(-y(w.x+b))); penalise_intercept = 1 for the liblinear
 *   solver (intercept is a penalised constant feature), 0 for lbfgs / newton-cg / sag / saga.  Stops on
 *   liblinear's relative gradient rule or, for the others, max|grad| <= tol * C (scikit-learn 0.22 hands
 *   tol to L-BFGS as gtol on objective / C).  iters_out = Newton steps.
 */
int psk_ridge_fit(psk_ctx *ctx, const float *X, const double *y, int n, int p, const int32_t *fold,
                  const double *fit_param, const int32_t *fit_fold, int n_fits, double *coef_out, double *icpt_out,
                  int32_t *iters_out);
int psk_logreg_l2_fit(psk_ctx *ctx, const float *X, const int32_t *y01, int n, int p, const int32_t *fold,
                      const double *fit_param, const int32_t *fit_fold, int n_fits, double tol, int max_iter,
                      int penalise_intercept, double *coef_out, double *icpt_out, int32_t *iters_out);

/* ---- f5: the `-bc SVM` estimator ------------------------------------------------------------------
 * Replaces GridSearchCV over SVC(kernel='linear' | 'rbf', probability=True, max_iter, tol) (set_model,
 * modeling.py:1025-1029, :1050-1056, :1086-1090).  Same batching and the same meaning of X, y01, n, p, fold,
 * fit_fold, n_fits as psk_logreg_l1_fit; fit_C[j] (and fit_gamma[j] for the rbf kernel) are fit j's parameters.
 * Per fit, libsvm's C-SVC dual  min 1/2 a'Qa - e'a, 0 <= a_i <= C, y'a = 0, Q_ij = y_i y_j K_ij  with class 0 as
 * libsvm's +1 (scikit-learn sorts the labels) and no class weights, walked by libsvm's Solver::Solve without
 * shrinking, step for step (WSS2 working sets with libsvm's tie rules, float Q entries, f64 elsewhere): a fit that
 * stops at max_iter returns that iterate, as scikit-learn does, so the PATH is part of the contract
 * (csrc/solver_svc.hip).  K: linear x_i . x_j, rbf exp(-gamma |x_i - x_j|^2).  max_iter = -1: no limit.
 *   dual_out[n_fits][n]  y_i alpha_i in libsvm's sign (class 0 positive), 0 for samples the fit did not train on
 *   rho_out[n_fits]
 *   dec_out[n_fits][n]   sum_j dual_j K(x_j, x_i) - rho for EVERY sample, held-out ones included (libsvm's sign:
 *                        scikit-learn's decision_function is its negative)
 *   iters_out[n_fits]    iterations taken (== max_iter: stopped at the limit); may be NULL
 * The sample x sample dot products are built once per call and shared by the fits (popcounts of bit-packed rows for
 * a 0/1 design, f64 dot products otherwise): at most 4096 samples (PSK_ERANGE beyond).  A fit whose training
 * samples are of one class is refused (PSK_EINVAL).  Decision values of rows that were not in the fit's X:
 * psk_svc_decision (f12), in the same operation order.
 */
int psk_svc_fit(psk_ctx *ctx, const float *X, const int32_t *y01, int n, int p, const int32_t *fold,
                const double *fit_C, const double *fit_gamma, const int32_t *fit_fold, int n_fits, int kernel,
                double tol, int max_iter, double *dual_out, double *rho_out, double *dec_out, int32_t *iters_out);

/* ---- f6: the `-bc DT` estimator -------------------------------------------------------------------
 * Replaces GridSearchCV over DecisionTreeClassifier() with {'max_depth': 1..10, 'criterion': ['gini', 'entropy']}
 * (set_model, modeling.py:1032-1033, :1069-1073, :1100-1103).  Same batching and the same meaning of X, y01, n, p,
 * fold, fit_fold, n_fits as psk_logreg_l1_fit; fit_max_depth[j] (1..10) and fit_criterion[j] (0 gini, 1 entropy)
 * are fit j's parameters.  Per fit, scikit-learn's depth-first best-split builder with its default settings on
 * the fit's training samples, nodes in pre-order (left subtree first; a clear bit goes left, the threshold is
 * 0.5), the proxy improvement in f64 with scikit-learn's expressions.  Among columns whose proxy is bit-equal the
 * LOWEST column index is taken (scikit-learn: the first in an unseeded random order); csrc/solver_tree.hip.
 *   node_count_out[n_fits], max_depth_out[n_fits]   nodes made, deepest level reached
 *   nodes_out[n_fits][PSK_TREE_NODE_CAP][6]          feature (-2: leaf), left, right (-1: leaf), n_node_samples,
 *                                                    n0, n1 (training samples of class 0 / 1 in the node)
 *   impurity_out[n_fits][PSK_TREE_NODE_CAP]          (of both, only the first node_count_out[j] slots of fit j are written)
 *   leaf_out[n_fits][n], frac_out[n_fits][n]         for EVERY sample, held-out ones included: the leaf it lands
 *                                                    in and that leaf's class-1 fraction n1 / n_node_samples
 * The design must be 0/1 (PSK_EINVAL otherwise); at most 4096 samples (PSK_ERANGE beyond).  A fit whose training
 * samples are of one class returns a single leaf.
 */
#define PSK_TREE_NODE_CAP 2047
int psk_tree_fit(psk_ctx *ctx, const float *X, const int32_t *y01, int n, int p, const int32_t *fold,
                 const int32_t *fit_max_depth, const int32_t *fit_criterion, const int32_t *fit_fold, int n_fits,
                 int32_t *node_count_out, int32_t *max_depth_out, int32_t *nodes_out, double *impurity_out,
                 int32_t *leaf_out, double *frac_out);

/* ---- f7: the `-bc RF` estimator -------------------------------------------------------------------
 * Replaces RandomizedSearchCV over RandomForestClassifier() with the seven-key grid of set_model (modeling.py:1030-1031,
 * :1057-1068, :1096-1099).  The contract is scikit-learn 1.7.2's forest for a given seed, to the node: the caller draws what
 * NumPy's RandomState draws and passes it in, the library builds the trees (csrc/solver_forest.hip), a workgroup building
 * one TREE at a time.  X, y01, n, p as for psk_tree_fit.  Per tree t:
 *   tree_weight[n_trees][n]    u16 sample weights (bootstrap multiplicities; 0 = not in the tree, which is also how a
 *                              held-out fold is expressed); at least one must be positive
 *   tree_state[n_trees]        state of the splitter's 32-bit xorshift (RandomState(seed_t).randint(0, 2^31 - 1))
 *   tree_fit[n_trees]          the fit (forest) the tree belongs to
 *   tree_export[n_trees]       != 0: the tree's node arrays are wanted
 * Per fit f: fit_criterion (0 gini, 1 entropy), fit_max_depth (0 = none), fit_max_features (columns visited per node, 1..p),
 * fit_min_samples_leaf (>= 1), fit_min_samples_split (>= 2).  Per tree, scikit-learn's depth-first builder over its
 * BestSplitter: the Fisher-Yates column walk with its constant-feature bookkeeping, the first column in visit order with a
 * strictly larger proxy, n_node_samples counting distinct in-bag samples, everything else weighted.
 *   sum0_out[n_fits][n], sum1_out[n_fits][n]   for EVERY sample: the class-0 / class-1 fractions of the leaves it lands in,
 *                                              added in tree order over the fit's trees (predict_proba x number of trees)
 *   node_count_out[n_trees], max_depth_out[n_trees]   nodes made, deepest level reached
 *   tree_node_off_out[n_trees]                 first slot of an exported tree in the node pool (-1: not exported); an
 *                                              exported tree reserves 2 x (samples of positive weight) - 1 slots, in tree
 *                                              order; node_pool is the pool's size in slots (PSK_ERANGE if too small)
 *   nodes_out[node_pool][6]                    feature (-2: leaf), left, right (-1: leaf), n_node_samples, w0, w1 (weighted
 *                                              class counts)
 *   impurity_out[node_pool]
 *   leaf_out[exported trees][n]                every sample's leaf, rows in tree order of the exported trees
 * (nodes_out / impurity_out / leaf_out may be NULL when no tree is exported.)  The design must be 0/1 (PSK_EINVAL
 * otherwise); at most 4096 samples (PSK_ERANGE beyond); a tree whose in-bag samples are of one class is a single leaf.
 */
int psk_forest_fit(psk_ctx *ctx, const float *X, const int32_t *y01, int n, int p, int n_trees,
                   const uint16_t *tree_weight, const uint32_t *tree_state, const int32_t *tree_fit,
                   const int32_t *tree_export, int n_fits, const int32_t *fit_criterion, const int32_t *fit_max_depth,
                   const int32_t *fit_max_features, const int32_t *fit_min_samples_leaf,
                   const int32_t *fit_min_samples_split, double *sum0_out, double *sum1_out, int32_t *node_count_out,
                   int32_t *max_depth_out, int64_t node_pool, int64_t *tree_node_off_out, int32_t *nodes_out,
                   double *impurity_out, int32_t *leaf_out);

/* ---- f9: `-bc DT` on k-mer counts (--real_counts) -------------------------------------------------
 * psk_tree_fit on a COUNT design: the reference fits DecisionTreeClassifier() on the count matrix under --real_counts
 * (modeling.py:1032-1033, :1069-1073, :1100-1103).  Arguments, limits and outputs as psk_tree_fit, except:
 *   X[n][p]   integers in 0 .. 2^24 (PSK_EINVAL on a negative, fractional, non-finite or larger value)
 *   threshold_out[n_fits][PSK_TREE_NODE_CAP]   the threshold at a split, -2.0 at a leaf (first node_count_out[j] slots)
 * Per node, _splitter.pyx::node_split_best of scikit-learn 1.7.2 on the float32 design: a column is constant in the node
 * when the node's training samples share one value; otherwise its candidates are the gaps between consecutive distinct
 * values present among them, in ascending order; the proxy and its strict comparison are psk_tree_fit's; the threshold is
 * lo / 2.0 + hi / 2.0 of the two values around the gap and x <= threshold goes left.  Among bit-equal proxies the LOWEST
 * column index wins, then the lowest threshold.  leaf_out / frac_out route EVERY sample by the reported thresholds.  On a
 * 0/1 design the result is psk_tree_fit's with every split threshold 0.5.  impurity_out (of all four tree calls) is taken on the
 * host from the node's class counts through the C library's log: scikit-learn's value to the bit.
 * The call makes one bit plane per gap between the distinct values of a column over all n samples: at most
 * PSK_TREE_PLANE_CAP planes (PSK_ERANGE beyond), 8 x ceil(n / 64) bytes of device memory each, next to the float design
 * (csrc/solver_tree_common.h).
 */
#define PSK_TREE_PLANE_CAP 1048576
int psk_tree_fit_counts(psk_ctx *ctx, const float *X, const int32_t *y01, int n, int p, const int32_t *fold,
                        const int32_t *fit_max_depth, const int32_t *fit_criterion, const int32_t *fit_fold, int n_fits,
                        int32_t *node_count_out, int32_t *max_depth_out, int32_t *nodes_out, double *impurity_out,
                        int32_t *leaf_out, double *frac_out, double *threshold_out);

/* ---- f10: `-bc RF` on k-mer counts (--real_counts) ------------------------------------------------
 * psk_forest_fit on a COUNT design (RandomForestClassifier() on the count matrix, modeling.py:1030-1031, :1057-1068,
 * :1096-1099).  Arguments, limits and outputs as psk_forest_fit; the design, the per-node search, the threshold and the
 * plane cap as psk_tree_fit_counts, with weighted counts in the proxy and min_samples_leaf on the distinct in-bag samples
 * of either side of a gap.  Ties: the first column in visit order wins, then the lowest threshold inside it; the
 * Fisher-Yates walk, the constant bookkeeping, the xorshift and n_node_samples are psk_forest_fit's.
 *   threshold_out[node_pool]   by node slot, as impurity_out: the threshold at a split, -2.0 at a leaf; may be NULL when
 *                              no tree is exported
 * sum0_out / sum1_out / leaf_out route EVERY sample, weight-0 ones included, by the reported thresholds.  On a 0/1
 * design the result is psk_forest_fit's with every split threshold 0.5.
 */
int psk_forest_fit_counts(psk_ctx *ctx, const float *X, const int32_t *y01, int n, int p, int n_trees,
                          const uint16_t *tree_weight, const uint32_t *tree_state, const int32_t *tree_fit,
                          const int32_t *tree_export, int n_fits, const int32_t *fit_criterion,
                          const int32_t *fit_max_depth, const int32_t *fit_max_features,
                          const int32_t *fit_min_samples_leaf, const int32_t *fit_min_samples_split, double *sum0_out,
                          double *sum1_out, int32_t *node_count_out, int32_t *max_depth_out, int64_t node_pool,
                          int64_t *tree_node_off_out, int32_t *nodes_out, double *impurity_out, int32_t *leaf_out,
                          double *threshold_out);

/* ---- f13: `-bc DT` / `-bc RF` on a real-valued design (--pca) --------------------------------------
 * psk_tree_fit_counts / psk_forest_fit_counts on a design of ANY finite float32 values: under --pca the reference fits its
 * tree models on the kept principal-component scores (modeling.py:1204, then set_model :1030-1033).  Arguments, limits and
 * outputs as the count calls (threshold_out included); what differs (csrc/solver_tree_real.hip):
 *   X[n][p]   float32, any finite value (PSK_EINVAL, naming the call, on a NaN or an infinity)
 * Equal values, as measured on scikit-learn 1.7.2 (its FEATURE_THRESHOLD of 1e-7 is not in effect in the search): any two
 * float32 values that compare different are different values.  A column is constant in a node when its in-bag values all
 * compare equal; a candidate is every place where the sorted in-bag values change (hi > lo as floats), adjacent float32 values
 * included; -0.0 and +0.0 are one value.  The threshold is (double)lo / 2.0 + (double)hi / 2.0, replaced by (double)lo if that
 * equals (double)hi or is infinite; (float32)x <= threshold goes left for every sample of the design.  Inside a column the first
 * strictly larger proxy in ascending order wins.  Proxy, min_samples_leaf, the walk over the columns, n_node_samples,
 * numbering and the reported impurities are the count calls'.  psk_tree_fit_real takes the LOWEST column index among
 * bit-equal proxies, which is scikit-learn's tree only where its seed does not matter; psk_forest_fit_real with one tree of
 * unit weights, max_features = p and tree_state = RandomState(s).randint(0, 2^31 - 1) is DecisionTreeClassifier(random_state=s).
 * On a 0/1 design the results are psk_tree_fit's / psk_forest_fit's with thresholds 0.5, on a count design the count calls' in
 * every output.
 * Memory rule: no bit planes and no plane cap.  Besides the float design the calls keep every column's sample order (u16)
 * and sorted values (f32), built once per call on the device: 6 n p bytes whatever the values; the search walks that order.
 */
int psk_tree_fit_real(psk_ctx *ctx, const float *X, const int32_t *y01, int n, int p, const int32_t *fold,
                      const int32_t *fit_max_depth, const int32_t *fit_criterion, const int32_t *fit_fold, int n_fits,
                      int32_t *node_count_out, int32_t *max_depth_out, int32_t *nodes_out, double *impurity_out,
                      int32_t *leaf_out, double *frac_out, double *threshold_out);
int psk_forest_fit_real(psk_ctx *ctx, const float *X, const int32_t *y01, int n, int p, int n_trees,
                        const uint16_t *tree_weight, const uint32_t *tree_state, const int32_t *tree_fit,
                        const int32_t *tree_export, int n_fits, const int32_t *fit_criterion,
                        const int32_t *fit_max_depth, const int32_t *fit_max_features,
                        const int32_t *fit_min_samples_leaf, const int32_t *fit_min_samples_split, double *sum0_out,
                        double *sum1_out, int32_t *node_count_out, int32_t *max_depth_out, int64_t node_pool,
                        int64_t *tree_node_off_out, int32_t *nodes_out, double *impurity_out, int32_t *leaf_out,
                        double *threshold_out);

/* ---- f8: the `-bc NB` estimator -------------------------------------------------------------------
 * set_model makes BernoulliNB() (modeling.py:1034-1035), but the REFERENCE CANNOT COMPLETE `-bc NB`: get_best_model
 * (:1075-1103) has no NB branch, best_model stays None (:623) and fit_model (:1216) fails on None.fit.  The yardstick is
 * therefore scikit-learn 1.7.2's BernoulliNB() with its default parameters, fitted directly, without a search
 * (csrc/solver_nb.hip).  The library counts and adds; the logarithms between the two calls are the caller's, taken on the
 * host in scikit-learn's own expressions, so that the fitted attributes are scikit-learn's bit for bit.
 *
 * psk_nb_fit: same batching and the same meaning of X, y01, n, p, fold, fit_fold, n_fits as psk_tree_fit (fit_fold[j] = -1:
 * all samples).  Per fit, over its training samples:
 *   feature_count_out[n_fits][2][p]   samples of class 0 / class 1 that carry the k-mer
 *   class_count_out[n_fits][2]        samples of class 0 / class 1
 * Integers, so the result is exact.  The design must be 0/1 (PSK_EINVAL otherwise); a fit whose training samples are of one
 * class is refused (PSK_EINVAL).
 *
 * psk_nb_jll: the joint log-likelihood of every row of X[n][p] (0/1, PSK_EINVAL otherwise) under n_models models:
 *   delta[n_models][2][p]          feature_log_prob_ - log(1 - exp(feature_log_prob_))
 *   class_log_prior[n_models][2]
 *   neg_sum[n_models][2]           sum over the columns of log(1 - exp(feature_log_prob_))
 *   jll_out[n_models][n][2]        ((sum over the columns j the row carries of delta[m][c][j]) + class_log_prior[m][c])
 *                                  + neg_sum[m][c]
 * in f64 without multiplications.  The order of the sum is part of the contract: 64 partial sums, partial sum l starting from
 * +0.0 and adding the set columns among l, l + 64, l + 128, ... in ascending order; then a_l = a_l + a_(l xor m) for m = 32,
 * 16, 8, 4, 2, 1 over all l at once, and a_0 is the sum.  A row's result depends on nothing but that row and the model.
 *
 * Limits of both calls (no sample x sample structure, so not the 4096 samples of the other fits): n <= 65535 x 64 =
 * 4,194,240 samples and at most 65535 fits or models per call (PSK_ERANGE beyond); every index is 64-bit, so n x p is
 * bounded only by the device memory that the float design of 4 n p bytes needs.
 */
int psk_nb_fit(psk_ctx *ctx, const float *X, const int32_t *y01, int n, int p, const int32_t *fold,
               const int32_t *fit_fold, int n_fits, int32_t *feature_count_out, int32_t *class_count_out);
int psk_nb_jll(psk_ctx *ctx, const float *X, int n, int p, const double *delta, int n_models,
               const double *class_log_prior, const double *neg_sum, double *jll_out);

/* ---- f11: `--pca`: principal components of the selected k-mers ---------------------------------------
 * PCA_analysis (modeling.py:1147-1206) runs StandardScaler().fit/transform and PCA().fit/transform on the k-mer columns;
 * prediction applies scaler.transform, pca_model.transform and [:, PCs_to_keep] (prediction.py:131-163).  The REFERENCE CANNOT
 * COMPLETE `--pca`: PCA_analysis calls self.t_test (:1184), which does not exist.  The yardstick is therefore scikit-learn
 * 1.7.2's StandardScaler() and PCA() with their defaults, which end in svd_flip(u_based_decision=False) (csrc/pca.hip).
 * All arithmetic is f64; both results are pure functions of the arguments (two calls give the same bits).
 *
 * psk_pca_fit: X[n][p] row-major, presence 0/1 or counts.  2 <= n <= 4096 (PSK_EINVAL below, PSK_ERANGE above), p >= 1,
 * 1 <= n_comp <= min(n, p) (PSK_EINVAL); a non-finite entry of X is PSK_EINVAL.
 *   mean_out[p]                column sum / n
 *   var_out[p]                 population variance (ddof 0): (sum_i (x - mean)^2) / n
 *   scale_out[p]               sqrt(var); 1 for a column that is constant over the samples (var 0)
 *   lambda_out[min(n, p)]      eigenvalues of Z Z', Z = (X - mean) / scale: the squared singular values of Z, descending,
 *                              clamped at 0
 *   scores_out[n][n_comp]      U S of the leading n_comp components
 *   components_out[n_comp][p]  S^-1 U' Z
 *   sweeps_out                 sweeps of the Jacobi eigen-solver (may be NULL)
 * Sign: in every component row the entry of largest magnitude is positive, the lowest column index deciding among bit-equal
 * magnitudes; the score column carries the same sign.  Rank floor: a component with lambda_i <= max(n, p) 2^-52 lambda_1 is
 * outside the numerical rank of the Gram matrix (numpy.linalg.matrix_rank's rule); its component row and its score column
 * are zeros.  The eigen-solver has a sweep cap: a fit that reaches it fails with PSK_ESTATE.
 *
 * psk_pca_transform: X[m][p], any m >= 1; center[p], scale[p], components[k][p]:
 *   scores_out[m][k]           scores[i][c] = sum_j ((X[i][j] - center[j]) / scale[j]) * components[c][j]
 * The caller passes center = scaler.mean_ + scaler.scale_ * pca.mean_ (a PCA whose mean_ is not zero is served too).  The
 * order of the sum is part of the contract: z_j = (X[i][j] - center[j]) / scale[j]; 64 partial sums, partial sum l starting
 * from +0.0 and adding the rounded products z_j * components[c][j] for j = l, l + 64, l + 128, ... in ascending order (a
 * multiplication, then an addition: nothing fused); then a_l = a_l + a_(l xor m) for m = 32, 16, 8, 4, 2, 1 over all l at
 * once, and a_0 is the sum.  A result depends on nothing but its row, its component, center and scale: transform(X[lo:hi])
 * equals transform(X)[lo:hi] bit for bit.
 */
int psk_pca_fit(psk_ctx *ctx, const float *X, int n, int p, int n_comp, double *mean_out, double *var_out,
                double *scale_out, double *lambda_out, double *scores_out, double *components_out,
                int32_t *sweeps_out);
int psk_pca_transform(psk_ctx *ctx, const float *X, int m, int p, const double *center, const double *scale,
                      const double *components, int k, double *scores_out);

/* ---- f14: the `--penalty L1+L2` regressor ---------------------------------------------------------------
 * Replaces GridSearchCV over ElasticNet(l1_ratio, max_iter, tol) (set_model, modeling.py:1003-1006; :1041 the alpha grid;
 * :1078-1080 the search).  The reference cannot finish this branch -- fit_model (:1211) tests the upper-cased penalty
 * against "elasticnet" --, so the model is scikit-learn's ElasticNet as set_model configures it.  Same batching as
 * psk_lasso_fit -- one workgroup per (alpha, fold) fit, refits included, one launch -- and the same meaning of X, y, n, p,
 * fold, fit_fold, n_fits, tol, max_iter and the outputs; fit_alpha[j] is fit j's alpha, l1_ratio is shared by the call and
 * must be finite and lie in [0, 1] (PSK_EINVAL otherwise; the context stays usable).
 * Objective, over the n training rows of a fit, intercept unpenalised (X, y centred by the training rows' means):
 *   (1/2n)||y - Xw - b||^2 + alpha l1_ratio ||w||_1 + 1/2 alpha (1 - l1_ratio) ||w||^2
 * walked as scikit-learn's enet_coordinate_descent walks it, so a fit that stops at max_iter returns that iterate:
 * with l1 = alpha l1_ratio n and l2 = alpha (1 - l1_ratio) n, cyclic sweeps over the columns of non-zero centred norm,
 *   tmp = X_j'R + w_j |X_j|^2,   w_j <- sign(tmp) max(|tmp| - l1, 0) / (|X_j|^2 + l2),   R updated at once.
 * Stop rule: after a sweep with w_max == 0 or d_w_max / w_max < tol, or the last sweep allowed, the duality gap
 *   dual = max|X'R - l2 w|,  c = l1 / dual if dual > l1 else 1,
 *   gap = (dual > l1 ? 1/2 R'R (1 + c^2) : R'R) + l1 ||w||_1 - c R'y + 1/2 l2 (1 + c^2) w'w
 * is evaluated and the descent ends when gap < tol y'y.  iters_out = sweeps as scikit-learn counts them (n_iter_).
 * intercept = mean y - sum_k mean_k w_k.  With l1_ratio = 1 every added term is an exact +0.0: the results are
 * psk_lasso_fit's bit for bit.  With l1_ratio = 0 the gap never closes and every fit runs max_iter sweeps, as scikit-learn's.
 * Routes and knobs are psk_lasso_fit's (PSK_NO_LASSO_COV, PSK_NO_LASSO_BITS, read per call): the covariance form for a 0/1
 * design of up to 4,096 samples and 1,024 columns, the four-wave bit-packed kernel for other 0/1 designs that fit its LDS,
 * the float kernel for everything else (--real_counts).  The kernels are the Lasso's, instantiated with the L2 term.
 * Device scratch for the duration of the call: as psk_lasso_fit -- the design in one orientation and the per-fit state; the
 * covariance form also takes the co-occurrence counts of every held-out fold, n_folds x 2 p^2 bytes (1.6 MB per fold at 907
 * columns; the form is skipped beyond 2 GiB).
 */
int psk_enet_fit(psk_ctx *ctx, const float *X, const double *y, int n, int p, const int32_t *fold,
                 const double *fit_alpha, const int32_t *fit_fold, int n_fits, double l1_ratio, double tol, int max_iter,
                 double *coef_out, double *icpt_out, int32_t *iters_out);

/* ---- f15: `-a/--assembly`: the k-mers of the model assembled into longer sequences --------------------------
 * Replaces kmer_assembler and its helpers (modeling.py:1526-1605; assembling, :1607-1622, writes the file).  The reference
 * compares every ordered pair of a round's strings in Python and never ends on a repeat; here a round's matching runs on the
 * device (csrc/asm.hip), the rest of the loop on the host (csrc/asm_host.h), and three caps end what cannot end by itself.
 * The reference as it runs appends NO reverse complements to its list: kmers_for_ML is set to {} (:585) and never filled, so
 * the map over it (:1572) is empty; both_strands chooses between the reference as it runs (0) and as it is written (1).
 *
 * Strings are packed two bits a base (A 0, C 1, G 2, T 3), 32 bases per u64, the first base in the two most significant bits
 * (a k-mer word of this ABI shifted up to the top of the word); string i is the ceil(len_bases[i] / 32) words from
 * words[word_off[i]] on; the unused low bits of its last word are not looked at.
 *
 * psk_asm_round: one round's matching over n strings (list positions 0 .. n - 1), 1 <= min_olap <= 31 (the reference's
 * k - 1), every string of min_olap .. 2^24 bases, n <= 2^24 (PSK_EINVAL / PSK_ERANGE otherwise).
 *   pairs_out[pair_cap][3]   (a, b, t) for every ordered pair of DIFFERENT list positions with an overlap: t is the largest
 *                            t with min_olap <= t <= min(|a|, |b|) and suffix_t(a) == prefix_t(b) (t == |a|: a is a prefix
 *                            of b; equal strings at two positions overlap by their length).  Order unspecified.
 *   n_pairs_out              the number of such pairs
 *   contained_out[n]         1 where string i is a substring of a string that differs from it, else 0
 * More than pair_cap pairs: PSK_ERANGE with a message naming pair_cap; n_pairs_out is still the true number, pairs_out holds
 * pair_cap of them, contained_out is complete, and the context stays usable.  n == 0: no pairs.  pair_cap <= 2^28.
 *
 * psk_assemble: the whole loop over n k-mers (2 <= k <= 32) given as 2k-bit words, as they are (not made canonical);
 * both_strands != 0 appends the reverse complement of every k-mer behind the list.  Per round, over the current list:
 * the strings inside a different string leave it; no pair left: stop; every string in no pair is emitted unless its reverse
 * complement has been emitted; the next list is the set of all a + b[t:].  At the stop the remaining strings are emitted
 * under the same rule.  Where the reference leaves the outcome to Python's set order this call has a rule: a round's list is
 * sorted by length, then lexicographically (A < C < G < T), and offered for emission in that order -- of a string and its
 * reverse complement the one of the earlier round wins, within a round the lexicographically smaller -- and the output is
 * sorted by length, longest first, lexicographically among equal lengths.  The set of min(s, reverse complement of s) over
 * the output is the reference's under every set order.
 *   text_out[text_cap]   the sequences in that order, separated by '\n' (none after the last, no NUL)
 *   n_seqs_out, text_len_out, rounds_out (may be NULL: rounds that merged something)
 * text_cap too small: PSK_ERANGE naming text_cap, n_seqs_out and text_len_out are set (call again with that much room).
 * n == 0: zero sequences.  Caps, read per call, each PSK_ERANGE with a message naming the knob and the round:
 *   PSK_ASM_MAX_STRINGS   strings in a round's list (deduplicated, before the contained ones leave), default 1,048,576
 *   PSK_ASM_MAX_PAIRS     overlapping pairs of a round (among the strings that stay), default 4,194,304
 *   PSK_ASM_MAX_LEN       bases of one string, default 65,535
 * The longest string at most doubles per round, so the length cap ends the endless growth of a repeat within about 13 rounds
 * of the defaults; the pair and string caps end exponential branching.  The context stays usable after any of them.
 * Device scratch for the duration of a round: the packed list, 28 bytes per string, 12 bytes per pair of the round's cap
 * (at most n (n - 1) pairs are reserved).
 */
int psk_asm_round(psk_ctx *ctx, const uint64_t *words, const uint64_t *word_off, const uint32_t *len_bases, int64_t n,
                  int min_olap, uint64_t pair_cap, int32_t *pairs_out, uint64_t *n_pairs_out, uint8_t *contained_out);
int psk_assemble(psk_ctx *ctx, const uint64_t *kmer_words, int64_t n, int k, int both_strands, char *text_out,
                 uint64_t text_cap, int64_t *n_seqs_out, uint64_t *text_len_out, int32_t *rounds_out);

/* ---- f12: decision values of a fitted SVM (prediction)---------------------------------------------
 * What libsvm's svm_predict_values computes for new rows, the one prediction whose cost grows with the training set
 * (rows x support vectors x k-mers for the rbf kernel):
 *   dec_out[m]   dec[i] = (sum_j coef[j] K(SV_j, X_i)) - rho, libsvm's sign; coef[j] = y_j alpha_j (the package's
 *                -dual_coef_[0]), SV[n_sv][p] the support vectors, X[m][p] the rows; kernel 0 linear, 1 rbf
 * The order of the operations is the contract, and it is the order of the loop that ends psk_svc_fit's solver kernel, so a
 * fit's dec_out and this call on the fit's support vectors (class 0 first, input order within a class) agree bit for bit:
 * d = SV_j . X_i, sa = SV_j . SV_j and sb = X_i . X_i are f64 sums over the columns in ascending order (a multiplication,
 * then an addition: nothing fused); K = d, or exp(-gamma * (sa + sb - 2 * d)); the sum starts from +0.0 and takes the
 * rounded products coef[j] * K for j = 0, 1, ..., n_sv - 1 one after the other; then rho is subtracted.  A result depends
 * on nothing but its row, the support vectors and the model: decision(X[lo:hi]) equals decision(X)[lo:hi] bit for bit.
 * When every entry of X and SV is 0 or 1 both are bit-packed and the dot products are popcounts; otherwise they are f64.
 * On 0/1 input both routes give the same bits (the sums are exact integers).  No sample x sample matrix is held, so there
 * is no 4096 cap: m >= 1, n_sv >= 1, p >= 1, every index is 64-bit.  PSK_EINVAL: a null buffer, a kernel other than 0 or
 * 1, a negative or non-finite gamma, a non-finite entry of X, SV, coef or rho.
 */
int psk_svc_decision(psk_ctx *ctx, const float *X, int m, int p, const float *SV, int n_sv, const double *coef,
                     double rho, int kernel, double gamma, double *dec_out);

/* ---- f16: `-bc XGBC` / `-reg XGBR`: gradient-boosted trees ------------------------------------------
 * The REFERENCE CANNOT COMPLETE either name: get_model_name, set_model, set_hyperparameters and get_best_model
 * (modeling.py:186-207, :994-1103) have no case for them.  The yardstick is scikit-learn 1.7.2's GradientBoostingClassifier()
 * / GradientBoostingRegressor() with their defaults, fitted directly, without a search (csrc/solver_gb.hip).  This is
 * scikit-learn's gradient boosting (friedman_mse trees on the residuals of log_loss / squared_error, subsample 1.0, every
 * feature considered, init None), NOT XGBoost's regularised objective.
 *
 * psk_gb_fit: X[n][p] 0/1, y[n] (0/1 for the log loss), fold / fit_fold / n_fits as psk_tree_fit (fit_fold[f] = -1: all
 * samples).  Per fit f the IN-BAG samples are those with fold[s] != fit_fold[f], all of weight 1; held-out samples are routed
 * and updated but never counted.  F is the raw prediction, F = init_raw[f] before stage 0 (the caller's: np.average(y) of the
 * in-bag samples for the squared error, log(q / (1 - q)) of their class-1 share clipped to [eps32, 1 - eps32] for the log loss).
 * Per stage:
 *   residuals  r_s = y_s - F_s (loss 0, squared error), r_s = y_s - gb_expit(F_s) (loss 1, log loss);
 *              gb_expit(x) = 1 / (1 + gb_exp(-x)), gb_exp this library's own function of IEEE +, -, *, /, rint and ldexp
 *              (csrc/solver_gb_math.h: clamp to [-708, 708], Cody-Waite reduction by ln 2 in two parts, the Taylor polynomial of
 *              degree 13 in Horner form, constants as hex floats), the same bits on the device, on the host and in NumPy
 *   sums       EVERY sum over samples is taken in a TWO-LEVEL ORDER: within a word of 64 samples (sample s lies in word s / 64)
 *              in ascending sample index from +0.0; then the word partials in ascending word index from +0.0
 *   a node     with in-bag set S: w = |S|, sum = sum r, sq = sum r r, value = sum / w,
 *              impurity = sq / w - (sum / w) * (sum / w).  A leaf when depth >= max_depth, or w < 2, or impurity <= DBL_EPSILON,
 *              or ALL r_s, s in S, ARE BIT-EQUAL (this library's rule: the case scikit-learn's leaf rule means and its rounding
 *              decides at random), or no column is non-constant in S
 *   a split    of a column j that is non-constant in S: w_r = set bits in S, w_l = w - w_r, sum_r = sum r over the set bits,
 *              sum_l = sum - sum_r, diff = w_r * sum_l - w_l * sum_r, proxy = diff * diff / (w_l * w_r)
 *              (FriedmanMSE.proxy_impurity_improvement).  The largest proxy wins, THE LOWEST COLUMN INDEX among bit-equal maxima
 *              (this library's rule; scikit-learn's random_state breaks such ties).  Nodes are numbered in pre-order, the left
 *              child (bit clear) first
 *   a leaf     loss 0: value as above.  loss 1 (_gb.py::_update_terminal_regions): with prob = y - r over S,
 *              num = (sum r) / w, den = (sum prob * (1 - prob)) / w, value = 0 if |den| < 1e-150 else num / den
 *   update     F_s += learning_rate * value[leaf(s)] for every sample
 * Every expression in f64, nothing fused.  PSK_GB_NODE_CAP(max_depth) slots per tree; outputs:
 *   node_count_out[n_fits][n_estimators]
 *   nodes_out[n_fits][n_estimators][cap][4]   feature (-2: leaf), left, right (-1: leaf), n_node_samples (in-bag)
 *   value_out / impurity_out[n_fits][n_estimators][cap]   (slots behind node_count are zero)
 *   raw_out[n_fits][n]                         F of every sample after the last stage
 *   staged_out[n_fits][n_estimators][n]        F of every sample after each stage; may be NULL
 * PSK_ERANGE: n > 4096 (a stage's residuals and the node masks live in LDS).  PSK_EINVAL: more than 65535 fits, max_depth outside 1..10,
 * n_estimators outside 1..1000, learning_rate not a finite number above 0, loss not 0 or 1, a non-finite y or init_raw, the log
 * loss with a y other than 0 / 1 or with a fit whose in-bag samples are of one class, a fit without in-bag samples, a design
 * value other than 0 or 1.
 *
 * psk_gb_decision: the raw predictions of the rows of X[n][p] (0/1, PSK_EINVAL otherwise; no sample cap) under one model in
 * psk_gb_fit's layout (node_count[n_estimators], nodes[n_estimators][cap][4], value[n_estimators][cap]):
 *   raw_out[n]   init_raw, then + learning_rate * value[leaf] stage after stage in stage order
 * which is psk_gb_fit's raw_out bit for bit on the fit's own rows.  PSK_EINVAL also for a tree that is not pre-order (a child
 * not behind its parent or outside node_count) or splits on a column outside 0 .. p - 1.
 *
 * psk_gb_fit_counts: psk_gb_fit on a COUNT design (`--real_counts`; the yardstick is the same scikit-learn estimator fitted on the
 * float32 count matrix).  X[n][p] holds integers in 0 .. 2^24 (PSK_EINVAL otherwise, in the words of psk_tree_fit_counts, which
 * name sample and column).  Every other argument, limit and refusal is psk_gb_fit's, and so is the arithmetic, with the columns
 * replaced by THRESHOLD PLANES:
 *   planes     built per call over all n samples (csrc/solver_tree_common.h, tree_pack_counts): a column with the distinct values
 *              g_0 < g_1 < ... has plane k with bit s = (x_sj >= g_(k+1)); planes are ordered by (column, k); a column that is
 *              constant over all samples has none.  More than PSK_TREE_PLANE_CAP planes: PSK_ERANGE
 *   candidate  a plane whose set bits within the node's in-bag set S number c with 0 < c < w.  w_r = c; sum_r = the sum of r over
 *              the plane's set bits in S, EACH PLANE'S SUM TAKEN ON ITS OWN in the two-level order (within a word of 64 samples
 *              ascending from +0.0, then the word partials ascending), never accumulated across the nested planes of a column;
 *              sum_l, diff and proxy as above
 *   winner     the largest proxy, THE LOWEST PLANE INDEX among bit-equal maxima.  Planes of one column that lie between the same
 *              two values present in S select the same samples and give bit-equal proxies, so the rule reads "lowest column, then
 *              lowest threshold": scikit-learn's walk over the gaps between the values present in the node
 *   threshold  lo / 2.0 + hi / 2.0, lo the largest value below the winning plane's g and hi the smallest value at or above it,
 *              both among the node's IN-BAG samples
 *   routing    the children's masks come from the plane k of that column with g_k <= threshold < g_(k+1) over all samples' values,
 *              not from the plane that won: a held-out sample whose value lies inside the gap goes by x <= threshold (a node with
 *              in-bag values {0, 3} splits at 1.5, a held-out 1 goes left)
 *   leaves     leaf rules, Newton leaf values, pre-order numbering, the update of F and the held-out rule are unchanged; a design
 *              without planes gives single-leaf stages
 * Outputs as psk_gb_fit, with nodes_out[..][0] the design COLUMN of a split (not the plane) and
 *   threshold_out[n_fits][n_estimators][cap]   the threshold at a split; -2.0 at a leaf and in the slots behind node_count
 * On a 0/1 design every output equals psk_gb_fit's and every split threshold is 0.5.
 *
 * psk_gb_decision_counts: psk_gb_decision for such a model, threshold[n_estimators][cap] beside nodes and value.  One thread per
 * sample reads the float design: X[s][feature] <= threshold goes left.  X must be a count design as above; no planes are made and
 * there is no sample cap.  PSK_EINVAL as psk_gb_decision, and for a split whose threshold is not finite.  On the fit's own rows
 * raw_out is psk_gb_fit_counts's raw_out bit for bit.
 */
#define PSK_GB_NODE_CAP(max_depth) ((2 << (max_depth)) - 1)
int psk_gb_fit(psk_ctx *ctx, const float *X, const double *y, int n, int p, const int32_t *fold, const int32_t *fit_fold,
               int n_fits, int loss, int n_estimators, double learning_rate, int max_depth, const double *init_raw,
               int32_t *node_count_out, int32_t *nodes_out, double *value_out, double *impurity_out, double *raw_out,
               double *staged_out);
int psk_gb_decision(psk_ctx *ctx, const float *X, int n, int p, int n_estimators, int max_depth, const int32_t *node_count,
                    const int32_t *nodes, const double *value, double init_raw, double learning_rate, double *raw_out);
int psk_gb_fit_counts(psk_ctx *ctx, const float *X, const double *y, int n, int p, const int32_t *fold, const int32_t *fit_fold,
                      int n_fits, int loss, int n_estimators, double learning_rate, int max_depth, const double *init_raw,
                      int32_t *node_count_out, int32_t *nodes_out, double *value_out, double *impurity_out,
                      double *threshold_out, double *raw_out, double *staged_out);
int psk_gb_decision_counts(psk_ctx *ctx, const float *X, int n, int p, int n_estimators, int max_depth,
                           const int32_t *node_count, const int32_t *nodes, const double *value, const double *threshold,
                           double init_raw, double learning_rate, double *raw_out);

/* ---- f1: fixed-dictionary counting (prediction) ---------------------------------------------
 * Replaces `gmer_counter -db <txt> <addr>` (prediction.Samples.map_samples, prediction.py:72-80):
 * occurrences, both strands with multiplicity, of each dictionary k-mer (canonical words) in
 * the file image.  counts_out[n_dict], in dictionary order.
 */
int psk_count_dict(psk_ctx *ctx, const uint8_t *bytes, size_t len, int k, const uint64_t *dict_words,
                   uint64_t n_dict, uint32_t *counts_out);
/* All samples of a prediction run against one dictionary (the Pool.map over samples of prediction.py:150-163):
 * the ingest of psk_count_kmers_batch (n_threads host threads move file bytes into pinned memory, FASTA and
 * FASTQ are framed on the GPU) with one dictionary kernel per sample and one read-back.  counts_out[n][n_dict].
 * _files: paths of UNCOMPRESSED files of sizes[i] bytes, read by the framing threads.  Any dictionary size: up to
 * 2048 words the table lives in LDS, beyond that in global memory (`--n_kmers 0` models). */
int psk_count_dict_batch(psk_ctx *ctx, int n, const uint8_t *const *bytes, const size_t *lens, int k,
                         const uint64_t *dict_words, uint64_t n_dict, uint32_t *counts_out, int n_threads);
int psk_count_dict_files(psk_ctx *ctx, int n, const char *const *paths, const size_t *sizes, int k,
                         const uint64_t *dict_words, uint64_t n_dict, uint32_t *counts_out, int n_threads);

/* ---- f2: MinHash sketch for the population-structure weights ---------------------------------
 * Replaces `mash sketch -r <addr> -o K-mer_lists/<name>` (Samples.get_mash_sketches,
 * modeling.py:386-390; bundled binary bin/mash 2.2): the `sketch_size` smallest distinct
 * MurmurHash3_x64_128(seed) hashes of the sample's canonical k-mers, ascending -- exactly the hash
 * list `mash info -d` prints.  Mash's defaults are k = 21, sketch_size = 1000, seed = 42.
 * hashes_out must hold sketch_size entries; *n_out receives how many were written.
 */
int psk_minhash_sketch(psk_ctx *ctx, const uint8_t *bytes, size_t len, int k, int sketch_size, uint32_t seed,
                       uint64_t *hashes_out, uint64_t *n_out);

/* Pairwise comparison of n bottom-s sketches (was `mash dist reference.msh reference.msh`,
 * Samples.get_mash_distances, modeling.py:411-421): for every pair the number of shared hashes and the
 * denominator of Mash's Jaccard estimate (the merge stops after sketch_size distinct union hashes).
 *   sketches[n][sketch_size]  ascending distinct hashes, rows padded; lens[n] = valid entries per row
 *   common_out[n][n], denom_out[n][n]  symmetric; the host turns them into Mash distances
 */
int psk_mash_pairs(psk_ctx *ctx, const uint64_t *sketches, const uint32_t *lens, int n, int sketch_size,
                   uint32_t *common_out, uint32_t *denom_out);

/* Neighbour joining of an n x n distance matrix (was Bio.Phylo.TreeConstruction.DistanceTreeConstructor.nj in
 * Samples.get_weights, modeling.py:447-458): the n - 2 joins in order.  Join t merges the clades at POSITIONS
 * mi_out[t] and mj_out[t] of the current clade list (the joined clade takes position mj, position mi is deleted),
 * with branch lengths d1_out[t] (clade mi) and d2_out[t] (clade mj); last_out = the distance left between the final
 * two clades.  Same arithmetic, scan order and tie-breaking as the library's scalar loops.  3 <= n <= 4096.
 */
int psk_nj_merges(psk_ctx *ctx, const double *dist, int n, int32_t *mi_out, int32_t *mj_out, double *d1_out,
                  double *d2_out, double *last_out);

/* ---- e: multi-GPU collectives (RCCL over xGMI, bound directly; librccl.so is opened on first use) ------------
 * The reference has no multi-process path (its parallelism is Pool(num_threads) over text chunks,
 * modeling.py:335-342, :660-675); these calls carry the three exchanges of the range-sharded path: the
 * all-reduce of the slab union sizes (the global Bonferroni denominator of modeling.py:644/:795), the
 * all-gather of the scan survivors and the all-to-all of list ranges (multi-GPU ingest).  One communicator per
 * context, on its own HIP stream.
 *   psk_comm_unique_id   rank 0: writes the 128-byte id of ncclGetUniqueId (returns its length); the caller's
 *                        rendezvous (a file, a socket) carries it to the other ranks
 *   psk_comm_init        every rank, same id: ncclCommInitRank on the context's GPU
 *   psk_comm_size        ncclCommCount of the communicator (>= 1; < 0 on error): what a multi-GPU measurement quotes
 *                        as proof that its collectives ran on RCCL with every rank joined
 *   psk_comm_allreduce   in place on `count` host values; dtype 0 = u64, 1 = f64; op 0 = sum, 1 = max
 *   psk_comm_allgather_host     recv[world][bytes] <- every rank's send[bytes] (host buffers, waited for)
 *   psk_comm_allgather_device   the same for DEVICE buffers, queued on the communicator's stream, not waited for
 *   psk_comm_alltoallv_device   send_counts[d] elements (elem_bytes 4 or 8) to rank d, back to back in send_dev;
 *                               recv_counts[s] elements from rank s, back to back in recv_dev; waited for
 *   psk_comm_stream      the communicator's hipStream_t (hand it to psk_export_survivors_async so that the
 *                        all-gather queued next is ordered behind the export on the device)
 *   psk_comm_sync        waits for everything queued on that stream
 */
int psk_device_count(void);
int psk_comm_unique_id(psk_ctx *ctx, uint8_t *id_out, int cap);
int psk_comm_init(psk_ctx *ctx, const uint8_t *id, int id_len, int rank, int world);
int psk_comm_size(psk_ctx *ctx);
int psk_comm_free(psk_ctx *ctx);
void *psk_comm_stream(psk_ctx *ctx);
int psk_comm_sync(psk_ctx *ctx);
int psk_comm_allreduce(psk_ctx *ctx, void *vals, int count, int dtype, int op);
int psk_comm_allgather_host(psk_ctx *ctx, const void *send, void *recv, uint64_t bytes);
int psk_comm_allgather_device(psk_ctx *ctx, const void *send_dev, void *recv_dev, uint64_t bytes);
int psk_comm_alltoallv_device(psk_ctx *ctx, const void *send_dev, const uint64_t *send_counts, void *recv_dev,
                              const uint64_t *recv_counts, int elem_bytes);
/* Plain device buffers for the callers of the exchanges (send / receive buffers live outside the context), and
 * waited-for copies: kind 0 host -> device, 1 device -> host, 2 device -> device; on_comm_stream != 0 orders the
 * copy behind the collectives queued on the communicator's stream. */
int psk_dev_alloc(psk_ctx *ctx, uint64_t bytes, void **out);
int psk_dev_free(psk_ctx *ctx, void *p);
int psk_dev_copy(psk_ctx *ctx, void *dst, const void *src, uint64_t bytes, int kind, int on_comm_stream);

/* ---- helpers shared with the host side ------------------------------------------------------ */
/* Host-only: the cleaned sequence stream the tokeniser hands to the GPU (bases kept, window
 * breaks collapsed to '\n', everything else dropped).  Returns the length written (<= len), or
 * a negative code.  Exposed for tests of the tokeniser contract. */
int64_t psk_frame_sequence(const uint8_t *bytes, size_t len, uint8_t *out, size_t out_cap);
/* The same stream as the GPU framing kernels produce it (the batch counters frame FASTA and FASTQ on the device,
 * csrc/frame_gpu.hip; r06: FASTQ that is not four lines per record too -- the scan of line kinds): identical except that
 * runs of window breaks are not collapsed.  Returns the length written.  For tests of the tokeniser contract. */
int64_t psk_frame_sequence_gpu(psk_ctx *ctx, const uint8_t *bytes, size_t len, uint8_t *out, size_t out_cap);

#ifdef __cplusplus
}
#endif
#endif /* PSK_H */
