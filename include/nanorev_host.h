/* nanorev_host.h - host-side helpers of the read path (libnanorev_host.so: plain C, no HIP, no GPU).
 *
 * The engine's callers cut a read into per-base events and compute each event's raw mean / standard deviation on
 * the host before the device call (the reference: nanorevutils/preprocessing.py:134-137, np.mean / np.std of
 * raw_signal[start:end] per base, inside signal_segmentation :85-170).  nrvh_event_stats is that loop in C with
 * NumPy's own summation order, so that the numbers are the ones NumPy gives, bit for bit
 * (tests/test_hoststage_golden.py compares it with np.mean / np.std event by event).
 */
#ifndef NANOREV_HOST_H
#define NANOREV_HOST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Replaces the per-base np.mean / np.std(ddof=0) of preprocessing.py:134-137.
 *   raw [n_raw]   the read's DAQ samples from its first event on (NanoReviser.py:120)
 *   starts [n_ev] event starts relative to raw[0], ascending; event i covers [starts[i], starts[i+1]), the last one
 *                 [starts[n_ev-1], starts[n_ev-1] + last_dur); ranges are clipped to n_raw like a Python slice
 *   mean, std [n_ev] f64 out; NaN for an empty range (what NumPy returns for an empty slice).
 * Returns 0, or -1 on bad arguments.  Pure function, thread-safe. */
int nrvh_event_stats(const int16_t* raw, int64_t n_raw, const int32_t* starts, int64_t n_ev, int32_t last_dur,
                     double* mean, double* std);

/* One single-read fast5 file -> the arrays of one read as the device call takes them (nrv_predict_reads_raw,
 * include/nanorev.h): what the reference's get_read_data (nanorevutils/nanorev_fast5_handeler.py:39-150), the medians
 * and per-base statistics of signal_segmentation (nanorevutils/preprocessing.py:100-101, 134-137) and the feature
 * rows of nanorevtrainutils.py:162-169 produce, read with an HDF5 subset written from the format specification
 * (csrc/nrv_host_fast5.c).  The Python host stage (h5lite.py + hoststage.py) is the definition: this gives the same
 * numbers bit for bit or declines.
 * All arrays are malloc'ed by the call and released by nrvh_free_read. */
typedef struct {
  int64_t n_raw;       /* samples from the read's first event on */
  int64_t n_ev;        /* bases */
  int16_t* raw;        /* [n_raw] */
  int32_t* starts;     /* [n_ev] event starts relative to raw[0] */
  float* feat;         /* [n_ev][6] color/300, mean/shift, std/scale, length/10, Albacore mean, Albacore stdv */
  char* bases;         /* [n_ev] + NUL: the basecalls (model_state letters) */
  double shift, scale; /* median and median absolute deviation of raw[] */
  char* fastq;         /* the file's Fastq record (NUL-terminated; NULL when absent or not asked for) */
  int64_t fastq_len;
} nrvh_read;

#define NRVH_OK 0
#define NRVH_UNSUPPORTED 1   /* not the subset this reader knows (pre-versioned basecaller output, another HDF5 layout,
                                a missing group, ...): run the Python host stage, which decides and words the error */
#define NRVH_E_READ 2        /* the reference's own failure for this file ("Events is too short ...", "Signal is shorter
                                than the Events"): the Python path raises the same */
#define NRVH_E_IO 3
#define NRVH_E_ARG 4

/* Returns NRVH_OK or one of the codes above with a short reason in err[err_len].  want_fastq != 0: also read the Fastq
 * record.  Thread-safe; touches no Python object (ctypes callers run it with the GIL released). */
int nrvh_load_fast5(const char* path, const char* group, const char* subgroup, int want_fastq, nrvh_read* out,
                    char* err, int err_len);
void nrvh_free_read(nrvh_read* r);

/* Several files -> the concatenated arrays of ONE device call (what cli._load_bundle builds): the reads that came
 * back NRVH_OK one behind the other in raw / starts / feat / bases, their (raw_len, ev_len, shift, scale) in meta, and
 * per file the status code with the reason for anything else (those files go through the Python host stage). */
#define NRVH_ERR_LEN 96
typedef struct {
  int32_t n_files, n_ok;
  int64_t n_raw, n_ev;   /* totals over the NRVH_OK reads */
  int16_t* raw;          /* [n_raw] */
  int32_t* starts;       /* [n_ev] relative to each read's own first sample */
  float* feat;           /* [n_ev][6] */
  char* bases;           /* [n_ev] + NUL */
  double* meta;          /* [n_files][4]: raw_len, ev_len, shift, scale (zeros where status != NRVH_OK) */
  int32_t* status;       /* [n_files] */
  char* fastq;           /* the Fastq records of the NRVH_OK reads one behind the other */
  int64_t* fastq_off;    /* [n_files + 1] offsets into fastq; -1: that file has no record */
  char* errors;          /* [n_files][NRVH_ERR_LEN] */
} nrvh_bundle;
int nrvh_load_bundle(const char* const* paths, int n, const char* group, const char* subgroup, int want_fastq,
                     nrvh_bundle* out);
void nrvh_free_bundle(nrvh_bundle* b);

/* The same two loaders for callers that leave the read statistics to the DEVICE (nrv_reads_raw_stats_begin, include/nanorev.h).
 * flags & NRVH_DEVICE_STATS: the median / MAD pass, the per-base mean / std pass and feature columns 1 - 2 are SKIPPED:
 * shift = scale = 0 and the two columns are 0 in what comes back, *device_stats (device_stats[i]) = 1.  A read with a base of
 * more than NRVH_DEVICE_STATS_MAX_BASE samples is declined: it comes back complete, as from nrvh_load_fast5, with the flag 0
 * (one GPU thread walks one base; a stalled pore must not hand it a million samples).  Everything else - status codes, raw,
 * starts, bases, columns 0, 3, 4, 5, the Fastq record - is what the plain loaders give.  flags = 0: the plain loaders.
 *   last_dur       samples of the read's last base (3 or 5), which the device needs for that base's statistics;
 *   bundle form    last_dur [n], device_stats [n] are the CALLER's arrays, one entry per file (0 where status != NRVH_OK).
 * Any of the three out-pointers may be NULL. */
#define NRVH_DEVICE_STATS 1
#define NRVH_DEVICE_STATS_MAX_BASE 16384
int nrvh_load_fast5_ex(const char* path, const char* group, const char* subgroup, int want_fastq, int flags, nrvh_read* out,
                       int32_t* last_dur, int32_t* device_stats, char* err, int err_len);
int nrvh_load_bundle_ex(const char* const* paths, int n, const char* group, const char* subgroup, int want_fastq, int flags,
                        nrvh_bundle* out, int32_t* last_dur, uint8_t* device_stats);

/* The calls of one read -> the revised read -> its output file: the merge of nanorevutils/output_handeler.py:83, 104-122
 * (decode as SURVEY.md 8a a16: model1 class = label, model2 class k = label k + 1; window i revises base
 * i + (T - 1) / 2), the record of output_handeler.py:26-62 byte for byte, written to a temporary and renamed to dst.
 *   bases [n_ev] the read's basecalls; a1, a2 [n_win] argmax of model1 / model2; qc [n_win] one Phred character per
 *   window for FASTQ (fastq != 0) or NULL; name: the record's name (file name, blanks replaced by "|||").
 * n_written: characters of the revised sequence. */
int nrvh_finish_read(const char* bases, int64_t n_ev, const int8_t* a1, const int8_t* a2, int64_t n_win, int T,
                     const uint8_t* qc, const char* name, const char* dst, int fastq, int64_t* n_written);

/* nrvh_finish_read for every read of ONE device call: bases / a1 / a2 / qc are the call's concatenated arrays (read r
 * has ev_len[r] bases and max(ev_len[r] - T, 0) windows; its window i is window e0 + i of the call, e0 = the bases in
 * front of it; n_win_total windows in all).  status[r] / n_written[r] per read; a failing read does not stop the others. */
int nrvh_finish_bundle(const char* bases, const int64_t* ev_len, int n_reads, const int8_t* a1, const int8_t* a2,
                       int64_t n_win_total, int T, const uint8_t* qc, const char* const* names, const char* const* dsts,
                       int fastq, int64_t* n_written, int32_t* status);

/* Revised reads that are ALREADY merged - what nrv_revise_reads_raw (include/nanorev.h) returns - to their output files: for
 * every read r of a call the record of output_handeler.py:26-62 byte for byte (the FASTQ writer's missing newline in front of
 * '+' included) from seq[off[r] .. off[r + 1]) and, for fastq != 0, qual over the same range ('#' per base when qual is NULL),
 * written to a temporary and renamed to dsts[r] exactly as nrvh_finish_bundle does.  names[r]: the record's name (file name,
 * blanks replaced by "|||").  n_seq: the bytes seq / qual hold; off [n_reads + 1].  status[r] / n_written[r] per read as for
 * nrvh_finish_bundle: a read whose offsets are not ascending or leave [0, n_seq] is NRVH_E_ARG, an unwritable destination
 * NRVH_E_IO; a failing read does not stop the others. */
int nrvh_write_records(const uint8_t* seq, const uint8_t* qual, int64_t n_seq, const int64_t* off, int n_reads,
                       const char* const* names, const char* const* dsts, int fastq, int64_t* n_written, int32_t* status);

/* thr[k - 2], k = 2 .. 40: the smallest f32 confidence c for which clip(round(-10 log10(max(1 - c, 1e-4))), 1, 40) - computed in
 * f64, rounded half to even: the command line's per-base quality - is at least k.  The q_thr table of nrv_revise_reads_raw for
 * callers without NumPy (cli.phred_thresholds finds the same 39 values from the NumPy formula itself). */
int nrvh_phred_thresholds(float thr[39]);

/* ABI version of this header (3: nrvh_load_fast5_ex / nrvh_load_bundle_ex). */
int nrvh_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
