/* nanorev.h - C-ABI of libnanorev_hip.so, the MI355X (gfx950) engine behind NanoReviser's
 * window reviser (model1 + model2).
 *
 * The reference has no FFI for this path; the seam it exposes is the pair of Keras callables
 * built by nanorevutils/output_handeler.py:206-255 (get_model1) and :258-307 (get_model2),
 *     Model(inputs=[signal_input (B,T,50,1) f32, read_input (B,T,6) f32], outputs=[(B,C) softmax])
 * (:250-251, :302-303), which NanoReviser.py:129-130 constructs per read and would call as
 * `model.predict([signal_x, read_x])`.  Each entry point below cites the reference interface
 * it stands in for.  INTEGRATION.md shows the ctypes stub a maintainer adds on the reference
 * side.
 *
 * Conventions: plain pointers and sizes only.  Every function returns 0 on success and a
 * negative nrv_status otherwise; nothing throws.  The engine copies weights at create time and
 * never keeps a caller pointer past the return of a call.  Calls on ONE handle are not
 * re-entrant (one caller at a time: two threads inside the same handle corrupt whole launch
 * groups); SEVERAL handles per (process, GPU) may be driven by several threads at once
 * (scripts/gpu_two_engines.py; the device is shared, so this buys overlap, not throughput).  There is NO CPU fallback: without a usable HIP device
 * nrv_create fails with NRV_E_NO_DEVICE.
 */
#ifndef NANOREV_H
#define NANOREV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nrv_handle nrv_handle;

typedef enum {
  NRV_OK = 0,
  NRV_E_INVALID = -1,    /* bad argument (null pointer, negative size, unsupported T) */
  NRV_E_WEIGHTS = -2,    /* weight blob does not have the size the graph requires */
  NRV_E_NO_DEVICE = -3,  /* no HIP device / device index out of range */
  NRV_E_HIP = -4,        /* a HIP runtime call failed; see nrv_last_error */
  NRV_E_NOMEM = -5
} nrv_status;

#define NRV_BACKEND_HIP 1

/* Flat little-endian f32 blob holding the 60 tensors of one model in Keras' positional
 * `load_weights` order (what `model.load_weights(<S>_win13_50ep_model{1,2}.h5)` would read;
 * path convention NanoReviser.py:191-193; order SURVEY.md Appendix A-11). */
typedef struct {
  const float* data;
  int64_t n_f32;
} nrv_weights;

/* Replaces get_model1()/get_model2() + load_weights (output_handeler.py:206-307;
 * NanoReviser.py:129-130).  T = window length (SENT_LEN, output_handeler.py:201; the shipped
 * weights are T=11).  recurrent_act: 0 = hard_sigmoid (Keras 2.2.4 default, what the weights
 * were trained with), 1 = sigmoid (Keras >= 2.3 behaviour, enviroment/NanoReviser_macOS.yaml). */
int nrv_create(const nrv_weights* model1, const nrv_weights* model2, int T, int device,
               int recurrent_act, nrv_handle** out);

void nrv_destroy(nrv_handle* h);

/* Replaces model1.predict([signal, read]) and model2.predict([signal, read])
 * (output_handeler.py:250-251, :302-303) on n independent windows.
 *   signal [n][T][50] f32, read [n][T][6] f32 (feature order nanorevtrainutils.py:169).
 *   p1 [n][6], p2 [n][5] softmax outputs; a1, a2 [n] argmax (ties -> lowest index).
 * Any output pointer may be NULL.  All pointers are HOST memory.
 * Alignment is C's: 4 bytes for the float arrays, 1 for a1 / a2; an array may be a view anywhere inside a larger one.
 * No byte outside the extents stated above is read into a result or written (nrv_predict_read likewise: the N events
 * in, N-T rows out).  Arrays of 4 MiB and more are page-locked in place for the call (whole pages around them, their
 * contents untouched) unless NRV_HOST_REGISTER=0 is in the environment. */
int nrv_predict(nrv_handle* h, const float* signal, const float* read, int64_t n,
                float* p1, float* p2, int8_t* a1, int8_t* a2);

/* Whole-read form: the sliding windows x[i:i+T], i in [0, N-T) of
 * nanorevtrainutils.py:198-209 are formed on the device and the signal branch runs once per
 * event instead of once per (window, timestep).
 *   sig_ev [N][50] f32, feat_ev [N][6] f32; outputs have N-T rows (0 rows if N <= T). */
int nrv_predict_read(nrv_handle* h, const float* sig_ev, const float* feat_ev, int64_t N,
                     float* p1, float* p2, int8_t* a1, int8_t* a2);

/* Whole reads from RAW samples: the signal segmentation of preprocessing.py:103-131 (per base the
 * 50 samples around its first sample, (x - shift)/scale, zero padded) runs on the device, so a read
 * crosses PCIe as int16 samples + int32 event starts + the 6 event features (~46 B per base instead
 * of 224).  Several reads can share one call: `raw` and the per-event arrays are the reads'
 * arrays concatenated, `reads[r]` says where read r lies in them and carries its shift / scale
 * (medians over the read, NanoReviser.py:120 -> preprocessing.py:99-100, computed by the caller).
 *   raw [n_raw] int16; starts [N] int32, relative to the first sample of their own read;
 *   feat_ev [N][6] f32.  Outputs: N - T rows, exactly those of nrv_predict_read on the
 *   concatenated per-event arrays (windows that straddle two reads are the caller's to skip). */
typedef struct {
  int64_t raw_off, raw_len;   /* samples of the read inside `raw` */
  int64_t ev_off, ev_len;     /* events of the read inside the per-event arrays */
  double shift, scale;
} nrv_read_desc;
int nrv_predict_reads_raw(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                          const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                          float* p1, float* p2, int8_t* a1, int8_t* a2);
/* The same call in two halves (r06), so that a caller can have the device work on call k+1 while it collects call k - what the
 * reference's per-read Pool tasks (NanoReviser.py:203-219) get from running several `predict` calls side by side:
 *   nrv_reads_raw_begin  copies the inputs (92 B per base) into page-locked staging - they may be freed or reused as soon as it
 *                        returns -, uploads them in one transfer and enqueues EVERY stage of the call; *ticket names the call;
 *   nrv_reads_raw_end    waits for that call's results and writes them to the p1 / p2 / a1 / a2 given to _begin (which must stay
 *                        valid until then; any may be NULL).  A call that tripped the f16x2 range guard is re-run whole on the
 *                        f32 kernels here (nrv_saturated's *reruns counts it).
 * At most two calls in flight per handle (a third _begin returns NRV_E_INVALID); calls complete in the order they began; between
 * a _begin and its _end only these two entry points may be called on the handle - and, the one exception, nrv_align_labels,
 * which works on a stream and a block of its own.  nrv_predict_reads_raw IS _begin + _end. */
int nrv_reads_raw_begin(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                        const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                        float* p1, float* p2, int8_t* a1, int8_t* a2, int* ticket);
int nrv_reads_raw_end(nrv_handle* h, int ticket);
/* The segmentation alone: sig_ev [N][50] f32 to HOST memory (what nrv_predict_reads_raw feeds the
 * signal branch; bit-identical to the host stage - used by the parity tests). */
int nrv_segment_reads(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts, int64_t N,
                      const nrv_read_desc* reads, int n_reads, float* sig_ev);

/* Raw reads whose STATISTICS are computed on the device as well (opt-in; nothing above changes): the read's shift / scale
 * (median and median absolute deviation of its samples, preprocessing.py:100-101) and, per base, the mean and standard
 * deviation of its samples (preprocessing.py:134-137) that feature columns 1 and 2 are made of
 * (mean / shift, std / scale; nanorevtrainutils.py:162-169).  The arguments of nrv_reads_raw_begin, plus per read
 *   last_dur [n_reads]   samples of the read's LAST base (3 or 5 in the reference, preprocessing.py:112-116); base e covers
 *                        [starts[e], starts[e+1]), the last one [starts[e], starts[e] + last_dur), clipped to raw_len;
 *   on_device [n_reads]  non-zero: reads[r].shift / .scale and columns 1 - 2 of the read's feat_ev rows are IGNORED and produced
 *                        on the device ahead of the call's first segmentation stage (the read needs 1 .. 2^32 - 1 samples);
 *                        zero: the read is used as given, exactly as by nrv_reads_raw_begin.
 * The numbers are the host stage's bit for bit (integer histograms; f64 sums in NumPy's pairwise order, no contraction; one
 * correctly rounded division each), so p1 / p2 / a1 / a2 are those of nrv_predict_reads_raw fed by the host stage, in every
 * precision mode.  One thread works through one base: callers keep reads with a base of more than 16 384 samples on the
 * host (libnanorev_host.so's loader does) - a cap on work, the results are right for any length.
 * nrv_reads_raw_end collects the call; tickets, the two-calls-in-flight rule and the range-guard re-run are those of
 * nrv_reads_raw_begin.  nrv_predict_reads_raw_stats IS _stats_begin + _end. */
int nrv_reads_raw_stats_begin(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                              const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                              const int32_t* last_dur, const uint8_t* on_device,
                              float* p1, float* p2, int8_t* a1, int8_t* a2, int* ticket);
int nrv_predict_reads_raw_stats(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                                const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                                const int32_t* last_dur, const uint8_t* on_device,
                                float* p1, float* p2, int8_t* a1, int8_t* a2);
/* The statistics alone, to HOST memory, by the kernels nrv_reads_raw_stats_begin runs (every read as if on_device; the shift /
 * scale of `reads` are ignored): shift, scale [n_reads]; mean, std [N] f64 (NaN for a base without samples);
 * feat12 [N][2] f32 = feature columns 1 and 2.  The twin of nrv_segment_reads, used by the parity tests. */
int nrv_read_stats(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts, int64_t N,
                   const nrv_read_desc* reads, int n_reads, const int32_t* last_dur, double* shift, double* scale,
                   double* mean, double* std, float* feat12);

/* Raw reads in, REVISED reads out (opt-in; nothing above changes): the merge of the two models' calls (output_handeler.py:83,
 * 104-122 as SURVEY.md 8a a16 decodes it), the per-base quality and the packing of the reads run on the device behind the
 * call's last launch group, and only the merged block crosses PCIe on the way back - p1 / p2 / a1 / a2 are not downloaded.
 * The arguments of nrv_reads_raw_stats_begin (last_dur and on_device may BOTH be NULL: statistics from the host, as for
 * nrv_reads_raw_begin), and instead of the four output arrays
 *   bases [N]       the reads' original basecalls (ASCII), concatenated like the per-event arrays;
 *   q_thr [39]      or NULL.  Entry k - 2 is the smallest f32 confidence min(p1[a1], p2[a2]) of a window that earns Phred k,
 *                   k = 2 .. 40 (ascending): its quality character is 33 + 1 + #{k : q_thr[k] <= confidence}, compared in f32.
 *                   nrvh_phred_thresholds (include/nanorev_host.h) gives the table of the command line's formula.  NULL (FASTA):
 *                   no quality is produced and `qual` is not touched;
 *   seq, qual       uint8, capacity N + max(N - T, 0) each (qual may be NULL): the revised reads back to back.  Event j of a read
 *                   with ev_len bases emits its own base with quality '#' for j < (T - 1) / 2 or j >= (T - 1) / 2 +
 *                   max(ev_len - T, 0); otherwise 0, 1 or 2 characters decided by its window's two argmax classes (both models agree
 *                   on a base: it; model1 'D' and model2 a base: the original base, then model2's; both '-': nothing; else the
 *                   original base), each with the window's quality.  Window i of a read is window ev_off + i of the call;
 *   off [n_reads + 1]  int64: read r is seq[off[r] .. off[r + 1]), off[n_reads] the total.
 * The bytes are those of the host merge (hoststage.emit_calls is the definition) on the outputs of nrv_predict_reads_raw, in
 * every precision mode.  N <= T: no window - seq is `bases`, qual all '#', nothing is enqueued.  N < 2^31.
 * nrv_reads_raw_end collects the call (seq / qual / off must stay valid until then); tickets, the two-calls-in-flight rule and the
 * range-guard re-run (which runs the merge again behind the f32 kernels) are those of nrv_reads_raw_begin.
 * nrv_revise_reads_raw IS _begin + _end. */
int nrv_revise_reads_raw_begin(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                               const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                               const int32_t* last_dur, const uint8_t* on_device, const uint8_t* bases, const float* q_thr,
                               uint8_t* seq, uint8_t* qual, int64_t* off, int* ticket);
int nrv_revise_reads_raw(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                         const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                         const int32_t* last_dur, const uint8_t* on_device, const uint8_t* bases, const float* q_thr,
                         uint8_t* seq, uint8_t* qual, int64_t* off);
/* The merge alone, by the kernels nrv_revise_reads_raw_begin runs, on calls the HOST supplies: bases [sum ev_len], ev_len [n_reads],
 * a1 / a2 [n_win] (any int8: labels are clipped to 0 .. 5 as the host merge does), p1 [n_win][6] / p2 [n_win][5] (needed only with
 * q_thr; the gather index is clamped to the row), n_win = max(sum ev_len - T, 0).  The twin of nrv_segment_reads / nrv_read_stats,
 * used by the parity tests. */
int nrv_merge_calls(nrv_handle* h, const uint8_t* bases, const int64_t* ev_len, int n_reads, const int8_t* a1, const int8_t* a2,
                    const float* p1, const float* p2, int64_t n_win, const float* q_thr, uint8_t* seq, uint8_t* qual, int64_t* off);

/* The same revised reads WITH a per-read revision report (opt-in; nothing above changes): what the merge did to each read,
 * counted on the device behind the merge - the only place where a call made this way still has p1 / p2 / a1 / a2.  The
 * arguments of nrv_revise_reads_raw_begin up to `off`, then
 *   tie_eps   a window is a near-tie when, for model 1 or model 2, NOT (top1 - top2 >= tie_eps), top1 / top2 the largest and the
 *             second largest value of its softmax row (a duplicated maximum gives 0; f32 arithmetic; a NaN row is a near-tie).
 *             4e-4 is what two precision modes that each meet the parity bar can differ by;
 *   report    uint64 [n_reads][NRV_REPORT_COLS], filled by nrv_reads_raw_end.  With o = (T - 1) / 2 and n_r = max(ev_len - T, 0),
 *             window i of a read revises its event o + i.  Columns, per read:
 *               0 bases_in = ev_len   1 windows = n_r   2 bases_out = off[r + 1] - off[r]   3 edge = ev_len - n_r (events kept as they are)
 *               4 confirmed    both models agree on a base, and it is the original one
 *               5 substituted  both models agree on a base, another one
 *               6 inserted     model1 'D', model2 a base: the original base plus model2's
 *               7 deleted      both '-': nothing emitted
 *               8 undecided    none of the three: the original base kept            (4 .. 8 add up to column 1)
 *               9 .. 14  histogram of model1's class clipped to 0 .. 5;  15 .. 19  of model2's class clipped to 0 .. 4
 *               20 agree2    windows whose model2 base (label a2 + 1 clipped to 0 .. 5) is the original base
 *               21 near_tie  see tie_eps
 *               22 q_sum     sum of (quality character - 33) over the read's output characters; 0 without q_thr / qual
 *               23 reserved, 0
 * hoststage.revision_report is the definition; the counts are integers, so the block is that function's on the outputs of
 * nrv_predict_reads_raw bit for bit, in every precision mode and whatever order the workgroups ran in.  seq / qual / off are
 * those of nrv_revise_reads_raw_begin.  N <= T: the report is filled on the host (edge = bases_in = bases_out = ev_len;
 * with a quality q_sum = 2 * ev_len, every character being '#', as the definition has it; everything else 0).
 * Tickets, the two-calls-in-flight rule, the failure paths and the range-guard re-run (which zeroes the block and counts again)
 * are those of nrv_revise_reads_raw_begin; `report` must stay valid until nrv_reads_raw_end.
 * nrv_revise_reads_raw_report IS _report_begin + _end. */
#define NRV_REPORT_COLS 24
int nrv_revise_reads_raw_report_begin(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                                      const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                                      const int32_t* last_dur, const uint8_t* on_device, const uint8_t* bases, const float* q_thr,
                                      uint8_t* seq, uint8_t* qual, int64_t* off, float tie_eps, uint64_t* report, int* ticket);
int nrv_revise_reads_raw_report(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                                const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                                const int32_t* last_dur, const uint8_t* on_device, const uint8_t* bases, const float* q_thr,
                                uint8_t* seq, uint8_t* qual, int64_t* off, float tie_eps, uint64_t* report);
/* nrv_merge_calls with the report, by the kernel nrv_revise_reads_raw_report_begin runs: p1 / p2 may be given without q_thr
 * (near_tie is then filled and q_sum 0); without p1 / p2 near_tie is 0.  The twin used by the parity tests. */
int nrv_merge_calls_report(nrv_handle* h, const uint8_t* bases, const int64_t* ev_len, int n_reads, const int8_t* a1, const int8_t* a2,
                           const float* p1, const float* p2, int64_t n_win, const float* q_thr, uint8_t* seq, uint8_t* qual, int64_t* off,
                           float tie_eps, uint64_t* report);

/* The same revised reads WITH a per-read edit list (opt-in; nothing above changes): WHICH bases the merge substituted, inserted
 * or deleted, where, and with what confidence - compacted in event order on the device behind the merge (and the report), the
 * only place where a call made this way still has p1 / p2 / a1 / a2.  The arguments of nrv_revise_reads_raw_report_begin up to
 * `report`, which may be NULL here (then no report is counted and tie_eps is ignored), then
 *   edits     nrv_edit [max(N - T, 0)]: at most one record per window.  Only the used prefix crosses PCIe and is written:
 *             records at and beyond edit_off[n_reads] are not touched;
 *   edit_off  int64 [n_reads + 1]: read r owns edits[edit_off[r] .. edit_off[r + 1]), ascending in pos_in; edit_off[n_reads] is
 *             the total.
 * With o = (T - 1) / 2, window i of a read revises its event o + i; one record for an event whose window is
 *   kind 1 substituted  both models agree on a base that is not the original one; alt = the agreed base
 *   kind 2 inserted     model1 'D', model2 a base; alt = model2's base, which sits at pos_out + 1 (pos_out is the kept original)
 *   kind 3 deleted      both '-'; alt = '-', pos_out = the position the next emitted character takes
 * (the rules of the report's columns 5 - 7); confirmed, undecided and edge events have none.  Fields:
 *   pos_in   the event's index inside its read (0-based position in the ORIGINAL read)
 *   pos_out  position inside the REVISED read (relative to off[r]) of the first character the event emitted
 *   ref      the original base (ASCII)
 *   qual     the window's quality character; 0 without q_thr / qual
 *   conf     v < u ? v : u with u = p1[w][clip(a1, 0, 5)], v = p2[w][clip(a2, 0, 4)]: the f32 operand the quality is computed
 *            from, copied, in FASTA calls too (p1 / p2 are in the call's output block either way)
 * hoststage.revision_edits is the definition; slots and positions are integer scans, so the records are that function's on the
 * outputs of nrv_predict_reads_raw bit for bit, in every precision mode and whatever order the workgroups ran in.  seq / qual /
 * off / report are those of nrv_revise_reads_raw_report_begin.  N <= T: edit_off is zeros, filled on the host.
 * Tickets, the two-calls-in-flight rule, the failure paths and the range-guard re-run (which runs the three launches again
 * behind the merge: plain stores, nothing accumulates) are those of nrv_revise_reads_raw_begin; `edits` and `edit_off` must
 * stay valid until nrv_reads_raw_end, which reads the total from the downloaded edit_off and fetches total x 16 bytes in a
 * second copy.  nrv_revise_reads_raw_edits IS _edits_begin + _end. */
typedef struct nrv_edit {
  uint32_t pos_in, pos_out;
  uint8_t kind, ref, alt, qual;
  float conf;
} nrv_edit;
#ifdef __cplusplus
static_assert(sizeof(nrv_edit) == 16, "nrv_edit is 16 bytes");
#else
_Static_assert(sizeof(nrv_edit) == 16, "nrv_edit is 16 bytes");
#endif
int nrv_revise_reads_raw_edits_begin(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                                     const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                                     const int32_t* last_dur, const uint8_t* on_device, const uint8_t* bases, const float* q_thr,
                                     uint8_t* seq, uint8_t* qual, int64_t* off, float tie_eps, uint64_t* report,
                                     nrv_edit* edits, int64_t* edit_off, int* ticket);
int nrv_revise_reads_raw_edits(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                               const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                               const int32_t* last_dur, const uint8_t* on_device, const uint8_t* bases, const float* q_thr,
                               uint8_t* seq, uint8_t* qual, int64_t* off, float tie_eps, uint64_t* report,
                               nrv_edit* edits, int64_t* edit_off);
/* nrv_merge_calls_report with the edit list, by the kernels nrv_revise_reads_raw_edits_begin runs: `report` may be NULL; p1 / p2
 * may be given without q_thr (conf is then filled and qual 0); without p1 / p2 conf is 0.  The twin used by the parity tests. */
int nrv_merge_calls_edits(nrv_handle* h, const uint8_t* bases, const int64_t* ev_len, int n_reads, const int8_t* a1, const int8_t* a2,
                          const float* p1, const float* p2, int64_t n_win, const float* q_thr, uint8_t* seq, uint8_t* qual, int64_t* off,
                          float tie_eps, uint64_t* report, nrv_edit* edits, int64_t* edit_off);

/* The same revised reads laid out as the BYTES OF AN OUTPUT FILE (opt-in; nothing above changes): one well-formed FASTA / FASTQ
 * record per read, packed on the device behind the merge (and the report / edit launches), so that a caller appends `blob` to a
 * file with one write and derives an index from rec_off.  The arguments of nrv_revise_reads_raw_edits_begin - `report` may be
 * NULL as there, `edits` / `edit_off` may both be NULL (no edit list), and `seq` / `qual` may be NULL (the merged reads are then
 * not handed back and do not cross PCIe; `off` is still filled) - then
 *   names     uint8 [name_off[n_reads]]: the record names, concatenated (no terminators); uploaded with the call's inputs;
 *   name_off  int64 [n_reads + 1]: read r's name is names[name_off[r] .. name_off[r + 1]); ascending from 0;
 *   blob      uint8 [name_off[n_reads] + q (N + max(N - T, 0)) + 3 q n_reads], q = 2 for FASTQ and 1 for FASTA: the capacity.  Only
 *             the used prefix crosses PCIe and is written: bytes at and beyond rec_off[n_reads] are not touched;
 *   rec_off   int64 [n_reads + 1]: read r owns blob[rec_off[r] .. rec_off[r + 1]); rec_off[n_reads] is the total.
 * With L = off[r + 1] - off[r] and nl the length of the name, a record is
 *   FASTA  '>' name '\n' seq '\n'                       nl + L + 3 bytes
 *   FASTQ  '@' name '\n' seq '\n' '+' '\n' qual '\n'    nl + 2 L + 6 bytes
 * without line wrapping; a read without bases has its record too (empty lines).  FASTQ or FASTA is decided by q_thr (non-NULL:
 * FASTQ), whether `qual` is handed back or not.  hoststage.pack_records is the definition: copies and integer offsets only, so
 * the bytes are that function's on the (seq, qual, off) of nrv_revise_reads_raw_begin, in every precision mode and whatever
 * order the workgroups ran in.  seq / qual / off / report / edits / edit_off are those of nrv_revise_reads_raw_edits_begin.
 * N <= T: nothing is enqueued; the records are formed on the host from `bases`, every quality '#'.  A call whose capacity
 * reaches 4 GiB is declined (NRV_E_INVALID).
 * Tickets, the two-calls-in-flight rule, the failure paths and the range-guard re-run (which runs the two launches again behind
 * the merge: plain stores, nothing accumulates) are those of nrv_revise_reads_raw_begin; `blob` and `rec_off` must stay valid
 * until nrv_reads_raw_end, which reads the total from the downloaded rec_off, checks it against the capacity and fetches
 * `total` bytes in a second copy, as it fetches the edit records.  nrv_revise_reads_raw_records IS _records_begin + _end. */
int nrv_revise_reads_raw_records_begin(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                                       const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                                       const int32_t* last_dur, const uint8_t* on_device, const uint8_t* bases, const float* q_thr,
                                       uint8_t* seq, uint8_t* qual, int64_t* off, float tie_eps, uint64_t* report,
                                       nrv_edit* edits, int64_t* edit_off, const uint8_t* names, const int64_t* name_off,
                                       uint8_t* blob, int64_t* rec_off, int* ticket);
int nrv_revise_reads_raw_records(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                                 const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                                 const int32_t* last_dur, const uint8_t* on_device, const uint8_t* bases, const float* q_thr,
                                 uint8_t* seq, uint8_t* qual, int64_t* off, float tie_eps, uint64_t* report,
                                 nrv_edit* edits, int64_t* edit_off, const uint8_t* names, const int64_t* name_off,
                                 uint8_t* blob, int64_t* rec_off);
/* The record launches alone, on merged reads the HOST supplies (what nrv_merge_calls returned): seq / qual uint8 [off[n_reads]]
 * (qual NULL: FASTA), off int64 [n_reads + 1] ascending from 0, names / name_off / blob / rec_off as above, the blob's capacity
 * being name_off[n_reads] + q off[n_reads] + 3 q n_reads.  The twin of nrv_merge_calls used by the parity tests. */
int nrv_pack_records(nrv_handle* h, const uint8_t* seq, const uint8_t* qual, const int64_t* off, int n_reads,
                     const uint8_t* names, const int64_t* name_off, uint8_t* blob, int64_t* rec_off);

/* The per-read QUALITY AND BASE PROFILE of the same revised reads (opt-in; nothing above changes): what a sequencing summary is
 * computed from - mean and median quality over the error probabilities, Q10 / Q20 / Q30 counts, base composition -, counted on
 * the device behind the merge (and the report / edit / record launches).  The arguments of nrv_revise_reads_raw_records_begin -
 * `report`, `edits` / `edit_off` and `seq` / `qual` may be NULL as there, and `names` / `name_off` / `blob` / `rec_off` may ALL be
 * NULL (no records; `seq` is then required as in nrv_revise_reads_raw_begin) - then
 *   prof_thr  float [39]: the thresholds the profile's qualities are computed with; the layout of q_thr and independent of it
 *             (q_thr alone still decides between FASTA and FASTQ);
 *   profile   uint64 [n_reads][NRV_PROFILE_COLS], one row per read:
 *     0 .. 41  output characters of the read whose quality q has clip(q - 33, 0, 41) == k;
 *     42 .. 46 output characters equal to 'A', 'C', 'G', 'T' (exact upper-case ASCII), and everything else;
 *     47       reserved, 0.
 *   Columns 0 .. 41 and columns 42 .. 46 each add up to off[r + 1] - off[r].
 * Both are required.  The profile is ALWAYS that of the FASTQ form of the call, whether a quality is written or not: a window's
 * quality is 33 + 1 + #{k : prof_thr[k] <= min(p1[clip(a1)], p2[clip(a2)])}, compared in f32, as in nrv_revise_reads_raw_begin;
 * an edge event has '#' (Phred 2).  hoststage.read_profile (on what hoststage.emit_calls returns for cli.phred_chars of the
 * call's outputs) is the definition; every counter is an integer, so the bytes do not depend on the order of the workgroups.
 * N <= T: nothing is enqueued; the block is filled on the host - column 2 is ev_len, the base counts are those of `bases`.
 * Tickets, the two-calls-in-flight rule, the failure paths and the range-guard re-run (which zeroes the block and counts again
 * behind the f32 kernels, as the report) are those of nrv_revise_reads_raw_begin; `profile` is filled by nrv_reads_raw_end,
 * downloaded with the call's block, and must stay valid until then.  nrv_revise_reads_raw_profile IS _profile_begin + _end. */
#define NRV_PROFILE_COLS 48
int nrv_revise_reads_raw_profile_begin(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                                       const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                                       const int32_t* last_dur, const uint8_t* on_device, const uint8_t* bases, const float* q_thr,
                                       uint8_t* seq, uint8_t* qual, int64_t* off, float tie_eps, uint64_t* report,
                                       nrv_edit* edits, int64_t* edit_off, const uint8_t* names, const int64_t* name_off,
                                       uint8_t* blob, int64_t* rec_off, const float* prof_thr, uint64_t* profile, int* ticket);
int nrv_revise_reads_raw_profile(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                                 const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                                 const int32_t* last_dur, const uint8_t* on_device, const uint8_t* bases, const float* q_thr,
                                 uint8_t* seq, uint8_t* qual, int64_t* off, float tie_eps, uint64_t* report,
                                 nrv_edit* edits, int64_t* edit_off, const uint8_t* names, const int64_t* name_off,
                                 uint8_t* blob, int64_t* rec_off, const float* prof_thr, uint64_t* profile);
/* nrv_merge_calls with the profile, by the kernel nrv_revise_reads_raw_profile_begin runs: p1 / p2 are required (NRV_E_INVALID
 * without them), q_thr may be NULL - a FASTA merge whose profile is still filled.  The twin used by the parity tests. */
int nrv_merge_calls_profile(nrv_handle* h, const uint8_t* bases, const int64_t* ev_len, int n_reads, const int8_t* a1, const int8_t* a2,
                            const float* p1, const float* p2, int64_t n_win, const float* q_thr, uint8_t* seq, uint8_t* qual, int64_t* off,
                            const float* prof_thr, uint64_t* profile);

/* SLIDING-WINDOW QUALITY TRIM AND LENGTH FILTER of the same revised reads (opt-in; nothing above changes): per read the part
 * worth keeping, found on the device behind the merge (and the report / edit launches) and AHEAD of the record launches, which
 * lay out the trimmed reads only.  The arguments of nrv_revise_reads_raw_profile_begin - `report`, `edits` / `edit_off`,
 * `seq` / `qual`, the records' four and `prof_thr` / `profile` (both or neither) may be NULL as there - then
 *   trim_thr  float [39]: the thresholds the trim's qualities are computed with; the layout of q_thr and independent of it;
 *   Q, W      the window rule: 1 <= Q <= 40, 1 <= W <= 64 (NRV_E_INVALID outside);
 *   min_len   >= 0: a read whose kept part is shorter has no record;
 *   trim      int64 [n_reads][2] = (lo, hi) per read.
 * The rule, integers only: read r has L = off[r + 1] - off[r] output characters with q[i] = Phred of character i - that of the
 * FASTQ form of the call, whether a quality is written or not: 1 + #{k : trim_thr[k] <= min(p1[clip(a1)], p2[clip(a2)])} for a
 * window, 2 for an edge event.  Position i is good when i + W <= L (a window never reaches into the next read) and
 * q[i] + ... + q[i + W - 1] >= Q * W; lo is the smallest good i, hi the largest good i plus W; no good position (L < W is one
 * case): lo = hi = 0.  hoststage.trim_bounds is the definition; minima and maxima of integers, so the bytes do not depend on the
 * order of the workgroups.
 * `seq` / `qual` / `off`, the report, the edit list and the profile describe the UNTRIMMED reads, as without the trim.  The
 * records are the exception: a read with hi - lo >= min_len has the record of seq[lo:hi] (and qual[lo:hi]), every other read is
 * DROPPED and has no record, rec_off[r + 1] == rec_off[r] (hoststage.pack_records with trim / min_len).  The blob's capacity is
 * that of the untrimmed call.
 * N <= T: nothing is enqueued; `trim` is filled on the host from the rule with every quality 2.  Tickets, the two-calls-in-flight
 * rule, the failure paths and the range-guard re-run (which starts the bounds from nothing behind the f32 kernels) are those of
 * nrv_revise_reads_raw_begin; `trim` is filled by nrv_reads_raw_end, downloaded with the call's block, and must stay valid until
 * then.  nrv_revise_reads_raw_trim IS _trim_begin + _end. */
int nrv_revise_reads_raw_trim_begin(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                                    const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                                    const int32_t* last_dur, const uint8_t* on_device, const uint8_t* bases, const float* q_thr,
                                    uint8_t* seq, uint8_t* qual, int64_t* off, float tie_eps, uint64_t* report,
                                    nrv_edit* edits, int64_t* edit_off, const uint8_t* names, const int64_t* name_off,
                                    uint8_t* blob, int64_t* rec_off, const float* prof_thr, uint64_t* profile,
                                    const float* trim_thr, int Q, int W, int64_t min_len, int64_t* trim, int* ticket);
int nrv_revise_reads_raw_trim(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                              const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                              const int32_t* last_dur, const uint8_t* on_device, const uint8_t* bases, const float* q_thr,
                              uint8_t* seq, uint8_t* qual, int64_t* off, float tie_eps, uint64_t* report,
                              nrv_edit* edits, int64_t* edit_off, const uint8_t* names, const int64_t* name_off,
                              uint8_t* blob, int64_t* rec_off, const float* prof_thr, uint64_t* profile,
                              const float* trim_thr, int Q, int W, int64_t min_len, int64_t* trim);
/* nrv_merge_calls with the trim, by the kernels nrv_revise_reads_raw_trim_begin runs: p1 / p2 are required, q_thr may be NULL.
 * names / name_off / blob / rec_off: all NULL, or the trimmed records as above (FASTQ by q_thr), the blob's capacity being
 * name_off[n_reads] + q (N + n_win) + 3 q n_reads.  The twin used by the parity tests. */
int nrv_merge_calls_trim(nrv_handle* h, const uint8_t* bases, const int64_t* ev_len, int n_reads, const int8_t* a1, const int8_t* a2,
                         const float* p1, const float* p2, int64_t n_win, const float* q_thr, uint8_t* seq, uint8_t* qual, int64_t* off,
                         const float* trim_thr, int Q, int W, int64_t min_len, int64_t* trim,
                         const uint8_t* names, const int64_t* name_off, uint8_t* blob, int64_t* rec_off);
/* The window and finish launches alone, on quality CHARACTERS the host supplies: qual uint8 [off[n_reads]] with
 * q[i] = max(qual[i] - 33, 0), off int64 [n_reads + 1] ascending from 0, trim int64 [n_reads][2].  The unit door of the window
 * kernel for arbitrary qualities. */
int nrv_trim_reads(nrv_handle* h, const uint8_t* qual, const int64_t* off, int n_reads, int Q, int W, int64_t* trim);
/* nrv_pack_records with a trim: trim int64 [n_reads][2] with 0 <= lo <= hi <= off[r + 1] - off[r] (NRV_E_INVALID otherwise) and
 * min_len >= 0, or trim NULL: nrv_pack_records' bytes. */
int nrv_pack_records_trim(nrv_handle* h, const uint8_t* seq, const uint8_t* qual, const int64_t* off, int n_reads,
                          const uint8_t* names, const int64_t* name_off, const int64_t* trim, int64_t min_len,
                          uint8_t* blob, int64_t* rec_off);

/* EDIT DISTANCE TO A TRUTH SET of the same reads (opt-in; nothing above changes): per read how far the original and the revised
 * read are from the true sequence the caller holds, found on the device by ONE launch behind everything else of the call.
 * The rule, integers only: d(t, s) is the global unit-cost edit distance of a truth t (m bytes) and a read s (n bytes):
 *   D[0][j] = j and D[i][0] = i;  D[i][j] = min(D[i-1][j] + 1, D[i][j-1] + 1, D[i-1][j-1] + c);
 *   c = 0 exactly when t[i-1] == s[j-1] and that byte is one of A C G T - any other byte (N, lower case, anything else) matches
 *   nothing, itself included;  d = D[m][n].  n = 0 gives d = m.  m = 0 means "this read has no truth": its row is all zeros
 *   and no distance is formed.
 * hoststage.edit_distance is the definition.  The arguments of nrv_revise_reads_raw_trim_begin - every block of it may be NULL
 * as there, and here the trim too: with trim == NULL the rule Q / W / min_len / trim_thr is not checked and no trim enqueued -
 * then, all three required,
 *   truth      uint8: the true sequences, one behind the other;
 *   truth_off  int64 [n_reads + 1] ascending from 0: read r has truth[truth_off[r] .. truth_off[r + 1]); no single truth of
 *              2^31 - 64 characters or more (NRV_E_INVALID);
 *   accuracy   uint64 [n_reads][NRV_ACCURACY_COLS]:
 *     0  truth_len
 *     1  dist_in  = d(truth, the original bases of the read)
 *     2  dist_out = d(truth, seq[off[r] .. off[r + 1])): the UNTRIMMED revision, as the report, the edits and the profile
 *     3  reserved, 0
 * One wave per (read, original | revised) pair; every word is a function of its pair alone, stored plainly: the bytes do not
 * depend on the order of the workgroups and the range-guard re-run accumulates nothing.  The truth travels with the call's one
 * input transfer; the caller's truth arrays are dead once _begin returns.  N <= T: nothing is enqueued, the block is filled
 * on the host with dist_out = dist_in.  Tickets, the two-calls-in-flight rule and the failure paths are those of
 * nrv_revise_reads_raw_begin; `accuracy` is filled by nrv_reads_raw_end.  nrv_revise_reads_raw_accuracy IS _accuracy_begin + _end. */
#define NRV_ACCURACY_COLS 4
int nrv_revise_reads_raw_accuracy_begin(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                                        const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                                        const int32_t* last_dur, const uint8_t* on_device, const uint8_t* bases, const float* q_thr,
                                        uint8_t* seq, uint8_t* qual, int64_t* off, float tie_eps, uint64_t* report,
                                        nrv_edit* edits, int64_t* edit_off, const uint8_t* names, const int64_t* name_off,
                                        uint8_t* blob, int64_t* rec_off, const float* prof_thr, uint64_t* profile,
                                        const float* trim_thr, int Q, int W, int64_t min_len, int64_t* trim,
                                        const uint8_t* truth, const int64_t* truth_off, uint64_t* accuracy, int* ticket);
int nrv_revise_reads_raw_accuracy(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                                  const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                                  const int32_t* last_dur, const uint8_t* on_device, const uint8_t* bases, const float* q_thr,
                                  uint8_t* seq, uint8_t* qual, int64_t* off, float tie_eps, uint64_t* report,
                                  nrv_edit* edits, int64_t* edit_off, const uint8_t* names, const int64_t* name_off,
                                  uint8_t* blob, int64_t* rec_off, const float* prof_thr, uint64_t* profile,
                                  const float* trim_thr, int Q, int W, int64_t min_len, int64_t* trim,
                                  const uint8_t* truth, const int64_t* truth_off, uint64_t* accuracy);
/* nrv_merge_calls with the accuracy block, by the kernel nrv_revise_reads_raw_accuracy_begin runs, on calls the host supplies.
 * The twin used by the parity tests. */
int nrv_merge_calls_accuracy(nrv_handle* h, const uint8_t* bases, const int64_t* ev_len, int n_reads, const int8_t* a1, const int8_t* a2,
                             const float* p1, const float* p2, int64_t n_win, const float* q_thr, uint8_t* seq, uint8_t* qual, int64_t* off,
                             const uint8_t* truth, const int64_t* truth_off, uint64_t* accuracy);
/* The same kernel on pairs the host supplies: pair k is the truth a[a_off[k] .. a_off[k + 1]) against the read
 * b[b_off[k] .. b_off[k + 1]); a_off / b_off int64 [n_pairs + 1] ascending from 0, no sequence of 2^31 - 64 characters or more
 * (NRV_E_INVALID); dist int64 [n_pairs], -1 for an empty truth.  The unit door of the kernel. */
int nrv_edit_distance(nrv_handle* h, const uint8_t* a, const int64_t* a_off, const uint8_t* b, const int64_t* b_off, int n_pairs,
                      int64_t* dist);

/* ERROR CLASSES AGAINST THE TRUTH SET (opt-in; nothing above changes): per read how many substitutions, insertions and
 * deletions separate the original and the revised read from the true sequence, found on the device by ONE launch behind
 * the accuracy's.  The rule, integers only, no traceback and no tie-break rule: for a truth t (m bytes) and a read s (n bytes),
 * bytes matching as above (equal, and one of A C G T; any other byte matches nothing, itself included), take among all global
 * alignments with the minimum number of edits d those with the largest number of matched columns, M.  (d, M) is unique and
 * follows from a forward recurrence over pairs compared lexicographically on (d, -M):
 *   W[0][j] = (j, 0) and W[i][0] = (i, 0);
 *   W[i][j] = min(W[i-1][j] + (1, 0), W[i][j-1] + (1, 0), W[i-1][j-1] + ((0, -1) on a match, (1, 0) otherwise));
 *   (d, -M) = W[m][n].  d is the d of the accuracy block.  n = 0 gives (m, 0).  m = 0 means "this read has no truth": its row
 *   is all zeros.
 * From the four integers: substitutions S = m + n - 2M - d, insertions (read characters absent from the truth) I = d - (m - M),
 * deletions (truth characters absent from the read) D = d - (n - M); M + S + I = n, M + S + D = m, S + I + D = d.
 * hoststage.edit_classes is the definition.  The arguments of nrv_revise_reads_raw_accuracy_begin - every block of it may be
 * NULL as there, and here `accuracy` too - then, required,
 *   errclass   uint64 [n_reads][NRV_ERRCLASS_COLS]:
 *     0  truth_len
 *     1  dist_in    2  match_in   = (d, M) of the truth and the original bases of the read
 *     3  dist_out   4  match_out  = (d, M) of the truth and seq[off[r] .. off[r + 1]): the UNTRIMMED revision
 *     5  reserved, 0
 * One wave per (read, original | revised) pair; every word is a function of its pair alone, stored plainly: the bytes do not
 * depend on the order of the workgroups and the range-guard re-run accumulates nothing.  N <= T: nothing is enqueued, the block
 * is filled on the host with out = in.  Tickets, the two-calls-in-flight rule and the failure paths are those of
 * nrv_revise_reads_raw_begin; `errclass` is filled by nrv_reads_raw_end.  nrv_revise_reads_raw_errclass IS _errclass_begin + _end. */
#define NRV_ERRCLASS_COLS 6
int nrv_revise_reads_raw_errclass_begin(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                                        const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                                        const int32_t* last_dur, const uint8_t* on_device, const uint8_t* bases, const float* q_thr,
                                        uint8_t* seq, uint8_t* qual, int64_t* off, float tie_eps, uint64_t* report,
                                        nrv_edit* edits, int64_t* edit_off, const uint8_t* names, const int64_t* name_off,
                                        uint8_t* blob, int64_t* rec_off, const float* prof_thr, uint64_t* profile,
                                        const float* trim_thr, int Q, int W, int64_t min_len, int64_t* trim,
                                        const uint8_t* truth, const int64_t* truth_off, uint64_t* accuracy, uint64_t* errclass, int* ticket);
int nrv_revise_reads_raw_errclass(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                                  const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                                  const int32_t* last_dur, const uint8_t* on_device, const uint8_t* bases, const float* q_thr,
                                  uint8_t* seq, uint8_t* qual, int64_t* off, float tie_eps, uint64_t* report,
                                  nrv_edit* edits, int64_t* edit_off, const uint8_t* names, const int64_t* name_off,
                                  uint8_t* blob, int64_t* rec_off, const float* prof_thr, uint64_t* profile,
                                  const float* trim_thr, int Q, int W, int64_t min_len, int64_t* trim,
                                  const uint8_t* truth, const int64_t* truth_off, uint64_t* accuracy, uint64_t* errclass);
/* nrv_merge_calls with the error-class block, by the kernel nrv_revise_reads_raw_errclass_begin runs, on calls the host
 * supplies.  The twin used by the parity tests. */
int nrv_merge_calls_errclass(nrv_handle* h, const uint8_t* bases, const int64_t* ev_len, int n_reads, const int8_t* a1, const int8_t* a2,
                             const float* p1, const float* p2, int64_t n_win, const float* q_thr, uint8_t* seq, uint8_t* qual, int64_t* off,
                             const uint8_t* truth, const int64_t* truth_off, uint64_t* errclass);
/* The same kernel on pairs the host supplies, as nrv_edit_distance takes them and refuses them; dist and match int64 [n_pairs],
 * -1 / -1 for an empty truth.  The unit door of the kernel. */
int nrv_edit_classes(nrv_handle* h, const uint8_t* a, const int64_t* a_off, const uint8_t* b, const int64_t* b_off, int n_pairs,
                     int64_t* dist, int64_t* match);

/* TRUTH REGIONS: INFIX ALIGNMENT ON BOTH STRANDS (opt-in; nothing above changes).  The accuracy and the error classes want the
 * exact true sequence of a read; a user has a reference and a mapper's approximate coordinates, so the truth is a REGION a few
 * bases long or short at each end, and half of them lie on the other strand.  This block places the original and the revised
 * read INSIDE its region, free ends on the region, on the forward strand or on both, by ONE launch behind the error classes'.
 * The rule, integers only, no traceback: for a region t (m bytes) and a read s (n bytes), bytes matching as above, take among
 * all substrings t[start:end] (0-based, half-open) the one with, in this order, the fewest edits d of a global alignment with
 * s, the most matched columns M, the largest start, the smallest end.  On the reverse strand t is first replaced by its
 * reverse complement (A<->T, C<->G; any other byte stays as it is and matches nothing) and start / end count on THAT.
 * (d, M, start, end) follows from a forward recurrence over triples compared lexicographically on (d, -M, -start):
 *   W[0][j] = (j, 0, 0) and W[i][0] = (0, 0, -i);
 *   W[i][j] = min(W[i-1][j] + (1, 0, 0), W[i][j-1] + (1, 0, 0), W[i-1][j-1] + ((0, -1, 0) on a match, (1, 0, 0) otherwise));
 *   (d, -M, -start, end) = the minimum over i = 0 .. m of (W[i][n], i).  n = 0 gives (0, 0, m, m).  m = 0 means "this read has
 *   no truth": its row is all zeros.
 * A cell is one signed 64-bit value d 2^42 - M 2^21 - start, so a region, and a read that has one, holds at most
 * NRV_INFIX_MAX_LEN characters: longer input is refused under the entry point's name (a REVISED read above it - the call
 * cannot know it beforehand - counts as empty).  hoststage.infix_classes is the definition.  The arguments of
 * nrv_revise_reads_raw_errclass_begin - every block of it may be NULL as there, `accuracy` and `errclass` too - then, required,
 *   strands    1: the forward strand alone; 2: both
 *   infix      uint64 [n_reads][NRV_INFIX_COLS]:
 *     0  truth_len     1  strands run (1 or 2)
 *     2 ..  5  dist, match, start, end of the ORIGINAL bases of the read on the forward strand
 *     6 ..  9  the same on the reverse strand (zeros with strands = 1)
 *    10 .. 13  of seq[off[r] .. off[r + 1]), the UNTRIMMED revision, on the forward strand
 *    14 .. 17  the same on the reverse strand (zeros with strands = 1)
 * One wave per (read, original | revised, forward | reverse) triple; every word is a function of its triple alone, stored
 * plainly: the bytes do not depend on the order of the workgroups and the range-guard re-run accumulates nothing.  N <= T:
 * nothing is enqueued, the block is filled on the host with out = in.  Tickets, the two-calls-in-flight rule and the failure
 * paths are those of nrv_revise_reads_raw_begin; `infix` is filled by nrv_reads_raw_end.  nrv_revise_reads_raw_infix IS
 * _infix_begin + _end. */
#define NRV_INFIX_COLS 18
#define NRV_INFIX_MAX_LEN 2097151 /* 2^21 - 1 */
int nrv_revise_reads_raw_infix_begin(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                                     const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                                     const int32_t* last_dur, const uint8_t* on_device, const uint8_t* bases, const float* q_thr,
                                     uint8_t* seq, uint8_t* qual, int64_t* off, float tie_eps, uint64_t* report,
                                     nrv_edit* edits, int64_t* edit_off, const uint8_t* names, const int64_t* name_off,
                                     uint8_t* blob, int64_t* rec_off, const float* prof_thr, uint64_t* profile,
                                     const float* trim_thr, int Q, int W, int64_t min_len, int64_t* trim,
                                     const uint8_t* truth, const int64_t* truth_off, uint64_t* accuracy, uint64_t* errclass,
                                     int strands, uint64_t* infix, int* ticket);
int nrv_revise_reads_raw_infix(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                               const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                               const int32_t* last_dur, const uint8_t* on_device, const uint8_t* bases, const float* q_thr,
                               uint8_t* seq, uint8_t* qual, int64_t* off, float tie_eps, uint64_t* report,
                               nrv_edit* edits, int64_t* edit_off, const uint8_t* names, const int64_t* name_off,
                               uint8_t* blob, int64_t* rec_off, const float* prof_thr, uint64_t* profile,
                               const float* trim_thr, int Q, int W, int64_t min_len, int64_t* trim,
                               const uint8_t* truth, const int64_t* truth_off, uint64_t* accuracy, uint64_t* errclass,
                               int strands, uint64_t* infix);
/* nrv_merge_calls with the infix block, by the kernel nrv_revise_reads_raw_infix_begin runs, on calls the host supplies.  The
 * twin used by the parity tests. */
int nrv_merge_calls_infix(nrv_handle* h, const uint8_t* bases, const int64_t* ev_len, int n_reads, const int8_t* a1, const int8_t* a2,
                          const float* p1, const float* p2, int64_t n_win, const float* q_thr, uint8_t* seq, uint8_t* qual, int64_t* off,
                          const uint8_t* truth, const int64_t* truth_off, int strands, uint64_t* infix);
/* The same kernel on pairs the host supplies (a: the regions, b: the reads), on ONE strand - reverse is 0 or 1; dist, match,
 * start and end int64 [n_pairs], -1 in all four for an empty region.  Offsets that do not ascend from 0, another `reverse` and
 * a length above NRV_INFIX_MAX_LEN are refused.  The unit door of the kernel. */
int nrv_infix_classes(nrv_handle* h, const uint8_t* a, const int64_t* a_off, const uint8_t* b, const int64_t* b_off, int n_pairs,
                      int reverse, int64_t* dist, int64_t* match, int64_t* start, int64_t* end);

/* PER-BASE TRAINING LABELS: THE TRUTH ALIGNMENT WITH ITS TRACEBACK (opt-in; nothing above changes).  The blocks above say how
 * far a read is from its truth in integers that need no traceback; the labels the two classifiers are trained on are the
 * per-base answer - which truth character stands opposite each read base, which read bases are inserted or followed by a
 * deletion - which the reference derives from an external mapper's SAM record (NanoReviser_train.py: parse_sam_record,
 * clean_read_map_ref, get_base_label).  With the infix block's placement of a read in its region, on either strand, the
 * alignment and its traceback are formed here.  hoststage.align_labels is the definition.
 * Per pair: a region t (m bytes), a read s (n bytes), reverse (0 or 1) and bounds 0 <= start <= end <= m;
 * u = strand(t)[start:end], L = end - start bytes; the strand and the matching of bytes as in the infix block.  The recurrence
 * is the error classes' on (u, s), cells (d, -M) compared lexicographically: G[0][j] = (j, 0), G[i][0] = (i, 0), and for
 * i, j >= 1 three candidates in this order: 0 the diagonal G[i-1][j-1] + ((0, -1) on a match, (1, 0) otherwise); 1 "I", the
 * read character alone, G[i][j-1] + (1, 0); 2 "D", the truth character alone, G[i-1][j] + (1, 0).  G[i][j] is their minimum,
 * dir[i][j] the FIRST candidate that attains it.  The path starts at (L, n) and, while i > 0 or j > 0, takes I if i == 0, D if
 * j == 0 and dir[i][j] otherwise; the columns visited, reversed, are the alignment.  Among all alignments with the optimal
 * (d, M) it is the one whose columns, read from the end backwards, are lexicographically smallest under diagonal < I < D: gaps
 * land left-aligned.
 *   labels   uint8 [b_off[n_pairs]], one byte per read base:
 *     bits 0 .. 2  the code of the column's truth character: 1 ("-") on an I column; on a diagonal column A 5, G 4, T 3, C 2
 *                  and 0 for any other byte - on the reverse strand of the complemented character
 *     bit 3 (8)    a diagonal column that is not a match
 *     bit 4 (16)   the next column or columns are D: the base is followed by deleted truth characters (a leading run of D,
 *                  in front of the first read base, flags nothing)
 *   summary  int64 [n_pairs][NRV_LABEL_COLS]:
 *     0 match   1 sub   2 ins   3 del (D columns, the leading ones included)
 *     4 clip_start  read bases in front of the first diagonal column, n when there is none
 *     5 clip_end    read bases behind the last diagonal column, 0 when there is none
 *     6 lead_del    D columns in front of the first read base
 * hoststage.label_strings gives the text forms: map (D if bit 4, else I if the code is 1, else X if bit 3, else M), label1 (0
 * if bit 4, else the code: model1's six classes) and label2 (the code: model2's five).  n = 0: no bytes and
 * (0, 0, 0, L, 0, 0, L); L = 0: every base is I; an EMPTY region, m = 0, means "no truth": -1 in all seven columns, zero bytes.
 * a: the regions, b: the reads, as nrv_infix_classes takes them; reverse, start and end per pair.  Refused under the entry
 * point's name, the handle staying usable: null arguments, offsets that do not ascend from 0, a reverse byte other than 0 or
 * 1, bounds outside the region, a read - or an end - start - above NRV_LABELS_MAX_LEN.
 * Two launches per batch of pairs (csrc/nrv_labels.h): the error classes' wavefront, one wave per pair, storing a 2-bit
 * direction per cell - ceil(L / 1024) (n + 63) 256 bytes of direction words per pair -, then one thread per pair walking back.
 * Pairs run in consecutive batches whose direction words fit 2 GiB (NRV_LABELS_BUDGET=<bytes>, read by nrv_create; a pair runs
 * alone if need be, 1.0 GiB at the most).  The block - inputs, carry words, direction words, outputs - is kept in the handle,
 * grown on demand and freed by nrv_destroy.  Plain stores, no atomics: the bytes do not depend on the batches.  Not timed yet.
 * The call runs on a non-blocking stream of its own and waits for that stream alone; it reads and writes nothing else of the
 * handle, so it MAY be called between a nrv_reads_raw_begin (or any other _begin) and its _end. */
#define NRV_LABEL_COLS 7
#define NRV_LABELS_MAX_LEN 65536 /* of a read and of end - start */
int nrv_align_labels(nrv_handle* h, const uint8_t* a, const int64_t* a_off, const uint8_t* b, const int64_t* b_off, int n_pairs,
                     const uint8_t* reverse, const int64_t* start, const int64_t* end, uint8_t* labels, int64_t* summary);

/* BOTH CLASSIFIERS SCORED AGAINST PER-BASE LABELS (opt-in; nothing above changes): what Keras' model.evaluate gives for this
 * pair of models - loss and accuracy per model, the confusion matrices, whether the confidence behind the Phred characters is
 * calibrated - and, per window, what the merge did to true errors and to correct bases.  The softmax rows of a merged call
 * never leave the device, so the join with the labels happens there, by ONE launch behind the merge (behind the report where
 * there is one).  hoststage.score_calls is the definition.  The arguments of nrv_revise_reads_raw_infix_begin - every block of
 * it may be NULL as there, and here the truth, `truth_off` and `infix` too: the score reads no truth - then, all three required,
 *   labels     uint8 [N], one byte per event of the call in nrv_align_labels' format (bits 0 .. 2 the code, bit 3 a non-match,
 *              bit 4 followed by deleted truth); the byte 0xFF means "unlabelled";
 *   score_thr  float [39] ascending: the thresholds of the calibration bins; the layout of q_thr and independent of it;
 *   score      uint64 [n_reads][NRV_SCORE_COLS], one row per read.
 * The rule, integers only.  Read r has n_r = max(ev_len - T, 0) windows; its window i is window w = ev_off + i of the call and
 * revises event j = (T - 1) / 2 + i of the read.  A window is LABELLED when its event's byte is not 0xFF and its code is
 * 1 .. 5; only labelled windows are counted.  Per labelled window, with a1 / a2 / p1 / p2 the call's own outputs at w:
 *   y1 = 0 if bit 4 else code (model 1's six classes), y2 = code - 1 (model 2's five); c1 = clip(a1, 0, 5), c2 = clip(a2, 0, 4);
 *   bin(p) = #{k : score_thr[k] <= p}, compared in f32 (bin b is Phred b + 1; a NaN lands in bin 0);
 *   decision d, on the UNCLIPPED x = a1, y = a2 + 1 as in the report: x == y and x >= 2: 0 confirmed where the base of label
 *     clip(x, 0, 5) ("D-CTGA") is the original base, 1 substituted where not; else x == 0 and y >= 2: 2 inserted; else
 *     x == 1 and y == 1: 3 deleted; else 4 undecided;
 *   kind k: 3 (D) if bit 4, else 2 (I) if code == 1, else 1 (X) if bit 3, else 0 (M).
 * Columns:
 *     0         windows n_r (stored once)          1  labelled windows
 *     2 ..  37  confusion of model 1: 2 + 6 y1 + c1
 *    38 ..  62  confusion of model 2: 38 + 5 y2 + c2
 *    63 .. 102  model 1 calibration: windows per bin(p1[w][c1]);   103 .. 142  those of them with c1 == y1
 *   143 .. 182  model 2 calibration: windows per bin(p2[w][c2]);   183 .. 222  those of them with c2 == y2
 *   223, 224    sum of nll16(p1[w][y1]), of nll16(p2[w][y2])
 *   225 .. 244  decision x kind: 225 + 4 d + k
 *   245         sub_right: d == 1 and clip(x, 0, 5) == code (the agreed base is the truth's)
 *   246, 247    reserved, 0
 * nll16(p) is -log2 p in units of 2^-16 bit, from the f32 bit pattern u by integers alone, e = (u >> 23) & 255, m = u & 0x7FFFFF:
 * the sign bit set, e == 0 or e == 255 (NaN, Inf, zero, denormals, negatives): 127 << 16; e >= 127 (p >= 1): 0; otherwise
 * y = 2^23 | m, f = 0, sixteen times { y = (y y) >> 23 in 64 bits; f <<= 1; if y >= 2^24 { f |= 1; y >>= 1 } } and
 * nll16 = ((127 - e) << 16) - f.  It exceeds -65536 log2 p by less than 2 (in its units).  The loss in nats, Keras' categorical
 * cross-entropy, is column 223 (224) x ln 2 / 65536 / column 1.
 * Every counter is an integer, so the bytes do not depend on the order of the workgroups.  The labels travel with the call's
 * one input transfer; the caller's `labels` and `score_thr` are dead once _begin returns.  N <= T: nothing is enqueued; the
 * block is filled on the host with zeros.  Tickets, the two-calls-in-flight rule, the failure paths and the range-guard re-run
 * (which zeroes the block and counts again behind the f32 kernels, as the report) are those of nrv_revise_reads_raw_begin;
 * `score` is filled by nrv_reads_raw_end, downloaded with the call's block, and must stay valid until then.
 * nrv_revise_reads_raw_score IS _score_begin + _end.  Not timed yet. */
#define NRV_SCORE_COLS 248
int nrv_revise_reads_raw_score_begin(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                                     const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                                     const int32_t* last_dur, const uint8_t* on_device, const uint8_t* bases, const float* q_thr,
                                     uint8_t* seq, uint8_t* qual, int64_t* off, float tie_eps, uint64_t* report,
                                     nrv_edit* edits, int64_t* edit_off, const uint8_t* names, const int64_t* name_off,
                                     uint8_t* blob, int64_t* rec_off, const float* prof_thr, uint64_t* profile,
                                     const float* trim_thr, int Q, int W, int64_t min_len, int64_t* trim,
                                     const uint8_t* truth, const int64_t* truth_off, uint64_t* accuracy, uint64_t* errclass,
                                     int strands, uint64_t* infix, const uint8_t* labels, const float* score_thr, uint64_t* score,
                                     int* ticket);
int nrv_revise_reads_raw_score(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                               const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                               const int32_t* last_dur, const uint8_t* on_device, const uint8_t* bases, const float* q_thr,
                               uint8_t* seq, uint8_t* qual, int64_t* off, float tie_eps, uint64_t* report,
                               nrv_edit* edits, int64_t* edit_off, const uint8_t* names, const int64_t* name_off,
                               uint8_t* blob, int64_t* rec_off, const float* prof_thr, uint64_t* profile,
                               const float* trim_thr, int Q, int W, int64_t min_len, int64_t* trim,
                               const uint8_t* truth, const int64_t* truth_off, uint64_t* accuracy, uint64_t* errclass,
                               int strands, uint64_t* infix, const uint8_t* labels, const float* score_thr, uint64_t* score);
/* nrv_merge_calls with the score, by the kernel nrv_revise_reads_raw_score_begin runs, on calls the host supplies: p1 / p2 may
 * be NULL (both: columns 63 .. 224 stay 0).  The twin used by the parity tests. */
int nrv_merge_calls_score(nrv_handle* h, const uint8_t* bases, const int64_t* ev_len, int n_reads, const int8_t* a1, const int8_t* a2,
                          const float* p1, const float* p2, int64_t n_win, const float* q_thr, uint8_t* seq, uint8_t* qual, int64_t* off,
                          const uint8_t* labels, const float* score_thr, uint64_t* score);

/* FITTING THE PER-WINDOW TAIL ON THE DEVICE (opt-in; nothing above changes): what Keras' model.fit gives for the layers behind
 * Flatten(main_out) - tensors 56 .. 59: feature.kernel Wf [6T][16], feature.bias bf [16], final_out.kernel Wo [16][C],
 * final_out.bias bo [C] - with the 56 tensors in front of them frozen (the reference: NanoReviser_train.py).  These four are the
 * only tensors that depend on T or on the class layout; weights.ModelWeights.with_window fills them with noise at T != the
 * shipped T.  The frozen backbone runs ONCE per window; its 6T main_out values stay on the device, and an epoch touches those
 * alone.  nanoreviser_amd/tailfit.py is the definition.  Not fitted here: anything in front of main_out (no backbone
 * gradients); and a fitted tail is not installed into the live handle - the caller writes a weight file and creates a new one.
 * THE SET.  Per model, flat f32 [rows][6T] (index t * 6 + k) and y uint8 [rows] in device memory, kept in the handle, grown on
 * demand, freed by nrv_destroy; at most NRV_FIT_MAX_ROWS rows (environment, read by nrv_create; default 2^24, 8.4 GB at T = 11).
 * Both models always hold the same rows.  A window is LABELLED as in the score block: labels are nrv_align_labels' bytes, one
 * per event, 0xFF = unlabelled; read r has max(ev_len - T, 0) windows, its window i revises event (T - 1) / 2 + i, and is
 * labelled when that event's byte is not 0xFF and its code (bits 0 .. 2) is 1 .. 5; y1 = 0 if bit 4 else code, y2 = code - 1.
 * Windows that straddle two reads are never added.
 *   nrv_fit_add_reads_raw  the inputs of nrv_reads_raw_stats_begin (last_dur / on_device may both be NULL: no device
 *     statistics) and labels uint8 [N]; synchronous.  The call's launch groups run on the NRV_PREC_F32 kernels WHATEVER the
 *     handle's precision mode (selected as the range guard's re-run selects them; in the f16x2 mode main_out never reaches
 *     memory), and behind each group's head launch a gather moves the six values per (row, t) of every labelled window to its
 *     slot: rows are appended in window order, slots from an integer prefix scan over the call's events.  Plain stores, no
 *     atomics.  *n_added = rows added; N <= T adds nothing.  A call that would pass the row cap is refused whole.
 *   nrv_fit_set_rows / nrv_fit_get_rows  replace the set by n host rows / read rows [first, first + count): the unit doors.
 *   nrv_fit_reset  empties the set (memory is kept);  nrv_fit_count  its rows (negative: an error code).
 * THE FIT, per model (0 or 1) with C = 6 or 5 classes.  Parameters travel as ONE vector of
 *   NRV_FIT_PARAMS(T, C) = 96T + 16 + 16C + C + 16C floats: [Wf | bf | Wo | bo | Ce], Ce [C][16] the centres.
 * Forward of a row F: z = F Wf + bf, f = max(z, 0), l = f Wo + bo, p = softmax(l) - in the operation order of the f32 mode's
 * tail, so p is what nrv_predict* returns in NRV_PREC_F32, bit for bit.  Loss of a batch of b rows (lstmmodel.py:63-74; class
 * weights multiply the row's cross-entropy, and the batch is divided by b):
 *   L = (1 / b) sum cw[y_i] (-ln p_i[y_i]) + lambda (1 / b) sum |f_i - Ce[y_i]|^2
 * Gradients with respect to all five tensors; the ReLU derivative is 1 exactly where z > 0.  Per batch two launches
 * (csrc/nrv_tailfit.h): one workgroup per 32 rows sums its rows in ascending order into a partial vector; one workgroup then
 * forms g = (sum of the partials in ascending order) / b and, unless some g is not finite, the Adam step of Keras 2.2.4 in f32,
 *   m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) (g g);  theta = theta - (lr_t m) / (sqrt(v) + eps),
 * every operation rounded on its own, sqrt and / correctly rounded, 1 - beta formed in f32, and
 *   lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t) computed on the host in f64 and rounded to f32, t counting from 1.
 * A batch with a non-finite g is SKIPPED: no update, t does not advance, it counts in `nonfinite` and in nothing else.
 * No atomics anywhere: the same calls give the same bytes.
 *   nrv_fit_begin   params NULL: the handle's own tensors 56 .. 59 and zero centres.  Resets m, v and t.  opts NULL: defaults
 *                   (B 512, lr 1e-3, beta 0.9 / 0.999, eps 1e-7, lambda 0.4, cw (3, 5, 1, 1, 1, 1) for model 0 and
 *                   (5, 1, 1, 1, 1) for model 1).  B in 1 .. NRV_FIT_MAX_BATCH.
 *   nrv_fit_grad    the reduced gradient g [NRV_FIT_PARAMS] of the batch `rows` [b] (row indices into the set) at the current
 *                   parameters, and its statistics; nothing is updated.  The unit door of the gradient kernel.
 *   nrv_fit_epoch   rows in the order of `order` [n], in consecutive batches of B, the last one short and divided by its own
 *                   size: 2 ceil(n / B) launches enqueued on the handle's stream with no host synchronisation in between.
 *                   Statistics are those BEFORE each batch's update, summed over the batches that were not skipped.
 *   nrv_fit_eval    forward only over `order` [n]; p [n][C] (may be NULL) and the statistics.  Updates nothing.
 *   nrv_fit_params  the current vector and t (either may be NULL).
 * nrv_fit_stats: rows; correct (argmax, ties to the lowest index, equal to the label); ce_sum = sum of cw[y] (-ln p[y]);
 * center_sum = sum of |f - Ce[y]|^2 (without lambda); steps (updates made); nonfinite (batches skipped - for nrv_fit_grad: 1 if
 * its g is not finite).  The sums are f64 sums of f32 terms.
 * Every nrv_fit_* call is refused with NRV_E_INVALID under its own name between a nrv_*_begin and its nrv_reads_raw_end, and
 * for null pointers, a model other than 0 / 1, a row index >= nrv_fit_count, b outside 1 .. NRV_FIT_MAX_BATCH, a label above
 * the class count, and nrv_fit_grad / _epoch / _eval / _params before nrv_fit_begin; the handle stays usable.
 * Timed (tools/fit_bench.py, one MI355X, 65 536 rows, B 512, T 11, nine epochs after three untimed): 17.06 M rows/s at tail depth
 * (17.01 .. 17.09), 1.452 M rows/s at head depth (1.451 .. 1.453; see the block below). */
#define NRV_FIT_MAX_BATCH 65536
#define NRV_FIT_PARAMS(T, C) (96 * (T) + 16 + 16 * (C) + (C) + 16 * (C))
typedef struct nrv_fit_opts {
  int32_t B;
  float lr, beta1, beta2, eps, lambda;
  float cw[6];
} nrv_fit_opts;
typedef struct nrv_fit_stats {
  int64_t rows, correct, steps, nonfinite;
  double ce_sum, center_sum;
} nrv_fit_stats;
int nrv_fit_reset(nrv_handle* h);
int64_t nrv_fit_count(nrv_handle* h);
int nrv_fit_add_reads_raw(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts, const float* feat_ev, int64_t N,
                          const nrv_read_desc* reads, int n_reads, const int32_t* last_dur, const uint8_t* on_device,
                          const uint8_t* labels, int64_t* n_added);
int nrv_fit_set_rows(nrv_handle* h, const float* flat1, const float* flat2, const uint8_t* y1, const uint8_t* y2, int64_t n);
int nrv_fit_get_rows(nrv_handle* h, int64_t first, int64_t count, float* flat1, float* flat2, uint8_t* y1, uint8_t* y2);
int nrv_fit_begin(nrv_handle* h, int model, const float* params, const nrv_fit_opts* opts);
int nrv_fit_grad(nrv_handle* h, int model, const uint32_t* rows, int b, float* grad, nrv_fit_stats* stats);
int nrv_fit_epoch(nrv_handle* h, int model, const uint32_t* order, int64_t n, nrv_fit_stats* stats);
int nrv_fit_eval(nrv_handle* h, int model, const uint32_t* order, int64_t n, float* p, nrv_fit_stats* stats);
int nrv_fit_params(nrv_handle* h, int model, float* params, int64_t* t);

/* ---- Fitting the whole head behind the frozen Bi-LSTMs: a second DEPTH of nrv_fit_* (opt-in) ----
 * At depth NRV_FIT_TAIL (the default) everything above holds as it stands.  At depth NRV_FIT_HEAD the frozen boundary moves
 * from main_out back to the output of lstm4: fitted are the three per-timestep dense layers - tensors 50 .. 55: dense1 W1
 * [128][128] b1 [128], dense2 W2 [128][32] b2 [32], main_out Wm [32][6] bm [6], every one behind a ReLU - and the tail's
 * tensors 56 .. 59 with the centres.  nanoreviser_amd/headfit.py is the definition.  Not fitted: the four Bi-LSTMs and the
 * signal branch.
 *   nrv_fit_set_depth  NRV_FIT_TAIL or NRV_FIT_HEAD (or NRV_FIT_LSTM4, below).  Refused by name unless the set is empty (call nrv_fit_reset first), and
 *                      between a nrv_*_begin and its nrv_reads_raw_end.  It forgets any nrv_fit_begin (the vector has another
 *                      length) and frees the other depth's set.     nrv_fit_depth  the current depth.
 * THE SET at head depth.  Per model x4 f32 [rows][T][128] - the f32 lstm4 output of the window, forward and backward halves
 * concatenated as the head kernels read them - and the same y arrays, grown on demand, freed by nrv_destroy; the flat main_out
 * rows are not kept.  A row is 512 T bytes, so the depth has its own cap: at most NRV_FIT_MAX_HEAD_ROWS rows (environment, read
 * by nrv_create; default 2^21, 11.8 GB at T = 11); a call that would pass it is refused whole, by that name.
 *   nrv_fit_add_reads_raw  unchanged signature and label rule; still the NRV_PREC_F32 kernels whatever the mode.  Behind each
 *     launch group a gather moves the T x 128 values of every labelled window, 16 bytes at a time with plain stores, from the
 *     head's input [tile][t][kq 32][32 rows][4] to the window's slot (slots from the same prefix scan).
 *   nrv_fit_set_rows_head / nrv_fit_get_rows_head  the unit doors at head depth, x [n][T][128].  The flat doors
 *     nrv_fit_set_rows / _get_rows are refused at head depth and the _head doors at tail depth, each under its own name; the
 *     handle stays usable.
 * THE FIT at head depth.  One vector of NRV_FIT_PARAMS_HEAD(T, C) = 20838 + NRV_FIT_PARAMS(T, C) floats:
 *   [W1 | b1 | W2 | b2 | Wm | bm | Wf | bf | Wo | bo | Ce]      kernels row-major [in][out]; the last five as the tail has them.
 * nrv_fit_begin, _grad, _epoch, _eval and _params take and return vectors of the CURRENT depth's length; params NULL at head
 * depth: the handle's own tensors 50 .. 59 and zero centres.  Forward of a row X [T][128], for every t:
 *   h1 = relu(X_t W1 + b1), h2 = relu(h1 W2 + b2), mo_t = relu(h2 Wm + bm), F[t * 6 + k] = mo_t[k], then the tail's forward
 * and loss - in the operation order of the f32 mode's head kernels (the same v_mfma_f32_32x32x2_f32 chains in the same k
 * order), so at the handle's own tensors nrv_fit_eval's p is what nrv_predict* returns in NRV_PREC_F32, bit for bit.
 * Backward, with the tail's dz [16]: dF = dz Wf^T, dmo_t = dF[t * 6 ..] where mo_t > 0, dh2 = dmo_t Wm^T where h2 > 0,
 * dh1 = dh2 W2^T where h1 > 0; the kernel gradients, summed over rows and t, are h2^T dmo, h1^T dh2, X_t^T dh1, the bias
 * gradients the column sums; the tail's five as above.  The 128- and 32-wide products run on the f32 matrix pipe; the backward
 * pass recomputes h1 and h2 of a timestep instead of keeping them (csrc/nrv_headfit.h).  Per batch three launches: the
 * gradient (at most 128 workgroups, each over its 32-row tiles in ascending order, one partial vector each), the reduction
 * g = (sum of the partials in ascending order) / b with the finite check, and the Adam step above, operation for operation,
 * which no parameter takes unless ALL of g is finite.  A batch with a non-finite g is skipped and counted as above.  Every
 * sum's order is a function of (b, T) alone and there are no atomics: the same calls give the same bytes.  nrv_fit_epoch
 * enqueues 3 ceil(n / B) launches with no host synchronisation in between.
 * A parameter count of the other depth cannot be passed (the vector's length is implied); the Python layer checks it. */
#define NRV_FIT_TAIL 0
#define NRV_FIT_HEAD 1
#define NRV_FIT_PARAMS_HEAD(T, C) (20838 + NRV_FIT_PARAMS(T, C))
int nrv_fit_set_depth(nrv_handle* h, int depth);
int nrv_fit_depth(nrv_handle* h);
int nrv_fit_set_rows_head(nrv_handle* h, const float* x1, const float* x2, const uint8_t* y1, const uint8_t* y2, int64_t n);
int nrv_fit_get_rows_head(nrv_handle* h, int64_t first, int64_t count, float* x1, float* x2, uint8_t* y1, uint8_t* y2);

/* ---- Fitting the last Bi-LSTM with the head: a third DEPTH of nrv_fit_* (opt-in) ----
 * At depth NRV_FIT_LSTM4 the frozen boundary moves back to the input of lstm4, the 256 -> 64 Bi-LSTM: fitted are its tensors
 * 44 .. 49 (164352 weights) and everything the head depth fits.  nanoreviser_amd/lstm4fit.py is the definition.  Not fitted:
 * lstm1 .. lstm3, the BatchNorms and the signal branch.  The number names the Bi-LSTM the fit starts at; 2 and 3 are refused.
 *   nrv_fit_set_depth  takes NRV_FIT_LSTM4 under the rules above (an empty set, nothing in flight; it forgets any nrv_fit_begin
 *                      and frees the other depths' sets).
 * THE SET at this depth.  Per model xb f32 [rows][T][256] - the BatchNorm (tensors 40 .. 43: xb = x sc + sh) of the f32 lstm3
 * output of the window, in input time order, as the f32 lstm4 launch reads it - and the same y arrays.  A row is 1024 T bytes;
 * the depth's own cap is NRV_FIT_MAX_LSTM4_ROWS (environment, read by nrv_create; default 2^20, 11.8 GB per model at T = 11); a
 * call that would pass it is refused whole, by that name.
 *   nrv_fit_add_reads_raw  unchanged signature and label rule; the NRV_PREC_F32 kernels whatever the mode.  Behind each launch
 *     group a gather moves the T x 256 values of every labelled window, 16 bytes at a time with plain stores, from lstm4's
 *     input [tile][t][kq 64][32 rows][4] to the window's slot (the f32 lstm3 launch has applied sc / sh in its epilogue).
 *   nrv_fit_set_rows_lstm4 / nrv_fit_get_rows_lstm4  the unit doors, xb [n][T][256].  Each depth's doors are refused at the
 *     other two depths under their own names; the handle stays usable.
 * THE FIT.  One vector of NRV_FIT_PARAMS_LSTM4(T, C) = 164352 + NRV_FIT_PARAMS_HEAD(T, C) floats:
 *   [W4f [256][256] | U4f [64][256] | b4f [256] | W4b | U4b | b4b | the head depth's vector]
 * row-major [in][out], gate columns in Keras order i, f, c, o, forward direction first.  params NULL: the handle's own tensors
 * 44 .. 59 as the file has them (no BatchNorm folded in) and zero centres.  Forward per direction over its own step order (the
 * backward direction walks t = T - 1 .. 0): z = xb_t W + h U + b, i f o = act(z) with the handle's recurrent_act, g = tanh(z),
 * c = f c + i g, h = o tanh(c); X4_t = [h_fw,t | h_bw,t], then the head depth's forward and loss.  Backward: dX4 = dh1 W1^T,
 * then back through time in both directions, act' decided on the forward VALUE (hard sigmoid: 0.2 exactly where 0 < a < 1);
 * gW = sum xb_t^T dz, gU = sum h_{s-1}^T dz, gb = sum dz (csrc/nrv_lstm4fit.h).  A batch runs in chunks of 4096 rows in
 * ascending order: forward, head (which also forms dX4), backward and the weight gradients are separate launches, then the
 * reduction and the Adam step of the head depth over the longer vector; the finite check covers the whole vector before any
 * parameter moves.  No atomics; every sum's order is a function of (b, T) alone: the same calls give the same bytes.
 * nrv_fit_epoch enqueues all launches with no host synchronisation in between; nrv_fit_eval runs the forward launches alone. */
#define NRV_FIT_LSTM4 4
#define NRV_FIT_PARAMS_LSTM4(T, C) (164352 + NRV_FIT_PARAMS_HEAD(T, C))
int nrv_fit_set_rows_lstm4(nrv_handle* h, const float* xb1, const float* xb2, const uint8_t* y1, const uint8_t* y2, int64_t n);
int nrv_fit_get_rows_lstm4(nrv_handle* h, int64_t first, int64_t count, float* xb1, float* xb2, uint8_t* y1, uint8_t* y2);

/* ---- Fitting the 192 -> 128 Bi-LSTM with everything behind it: a fourth DEPTH of nrv_fit_* (opt-in) ----
 * At depth NRV_FIT_LSTM3 the frozen boundary moves back to the input of lstm3, the Bi-LSTM where the read branch and the signal
 * branch meet: fitted are its tensors 34 .. 39 (328704 weights) and everything the lstm4 depth fits (tensors 44 .. 59 and the
 * centres).  nanoreviser_amd/lstm3fit.py is the definition.  Frozen: tensors 0 .. 33 (lstm1, lstm2, the signal branch) AND the
 * BatchNorm between lstm3 and lstm4 (tensors 40 .. 43), which lies inside the fitted section and is applied in its inference
 * form, Xb4 = h3 * sc + sh (one f32 multiply, one f32 add, sc / sh from the moving statistics as the handle holds them).  A
 * STATED DEVIATION: Keras in training phase would normalise with the batch's statistics and fit gamma and beta; this depth
 * fine-tunes with the moving statistics fixed.  The constant is 8: 2, 3, 5, 6, 7, 9 and -1 stay refused.
 *   nrv_fit_set_depth  takes NRV_FIT_LSTM3 under the rules above.
 * THE SET at this depth.  Per model x f32 [rows][T][192] - the BatchNorm'd f32 lstm2 output of the window (128 values), then
 * signal_x_out (64 values), in the order of the model's concatenate, as the f32 lstm3 launch reads them - and the same y
 * arrays.  A row is 768 T bytes; the depth's own cap is NRV_FIT_MAX_LSTM3_ROWS (environment, read by nrv_create; default 2^20,
 * 8.9 GB per model at T = 11); a call that would pass it is refused whole, by that name.
 *   nrv_fit_add_reads_raw  unchanged signature and label rule; the NRV_PREC_F32 kernels whatever the mode.  INSIDE each launch
 *     group - behind the lstm2 launch and the signal branch, in front of the lstm4 launch, whose output overwrites lstm2's - a
 *     gather moves the T x 192 values of every labelled window, 16 bytes at a time with plain stores, through the two views the
 *     f32 lstm3 launch reads to the window's slot.  The group then runs to its end as at every depth.
 *   nrv_fit_set_rows_lstm3 / nrv_fit_get_rows_lstm3  the unit doors, x [n][T][192].  Each depth's doors are refused at the
 *     other depths under their own names; the handle stays usable.
 * THE FIT.  One vector of NRV_FIT_PARAMS_LSTM3(T, C) = 328704 + NRV_FIT_PARAMS_LSTM4(T, C) floats:
 *   [W3f [192][512] | U3f [128][512] | b3f [512] | W3b | U3b | b3b | the lstm4 depth's vector]
 * row-major [in][out], gate columns i, f, c, o, forward direction first.  params NULL: the handle's own tensors 34 .. 39 and
 * 44 .. 59 as the file has them and zero centres.  Forward: lstm3 as lstm4 above with H = 128, H3_t = [h_fw,t | h_bw,t],
 * Xb4 = H3 sc + sh, then the lstm4 depth's forward and loss.  Backward: the lstm4 depth's, then dX3 = (sum over both
 * directions, forward first, of dz4 W4^T) * sc, then back through time in lstm3 with dh = dX3_t[direction's half] +
 * dz_{s+1} U3^T; gW3 = sum x_t^T dz, gU3 = sum h_{s-1}^T dz (raw h; exactly zero at T = 1), gb3 = sum dz
 * (csrc/nrv_lstm3fit.h).  Chunks, reduction, finite check and Adam step as at lstm4 depth over the longer vector; no atomics,
 * the same calls give the same bytes.  nrv_fit_eval runs the forward launches alone. */
#define NRV_FIT_LSTM3 8
#define NRV_FIT_PARAMS_LSTM3(T, C) (328704 + NRV_FIT_PARAMS_LSTM4(T, C))
int nrv_fit_set_rows_lstm3(nrv_handle* h, const float* x1, const float* x2, const uint8_t* y1, const uint8_t* y2, int64_t n);
int nrv_fit_get_rows_lstm3(nrv_handle* h, int64_t first, int64_t count, float* x1, float* x2, uint8_t* y1, uint8_t* y2);

/* ---- Fitting the signal branch with lstm3 and everything behind it: a fifth DEPTH of nrv_fit_* (opt-in) ----
 * At depth NRV_FIT_SIGNAL the part of the model that reads the raw current is fitted: conv1.kernel [3][1][8] and .bias (tensors
 * 0, 1), conv2.kernel [3][8][8] and .bias (6, 7), sig_dense.kernel [400][64] and .bias (32, 33) - 25896 weights - and everything
 * the lstm3 depth fits (34 .. 39, 44 .. 59 and the centres).  nanoreviser_amd/signalfit.py is the definition.  Frozen: lstm1,
 * lstm2 and their BatchNorms (12 .. 31) AND the three BatchNorms inside the fitted section (2 .. 5, 8 .. 11, 40 .. 43).  TWO STATED
 * DEVIATIONS: those three BatchNorms are applied in their inference form from the moving statistics as the handle holds them
 * (behind a convolution relu(conv) * s + h, one f32 multiply and one f32 add), where Keras in training phase would normalise
 * with the batch's statistics and fit gamma and beta; and the reference's Dropout(0.2) behind the identity block is not applied -
 * a deviation that holds only while nrv_fit_set_dropout (below) is off.
 * The constant is 16: 2, 3, 5, 6, 7, 9 .. 15, 17 and -1 stay refused.
 *   nrv_fit_set_depth  takes NRV_FIT_SIGNAL under the rules above.
 * THE SET at this depth.  Per model x2 f32 [rows][T][128] - the BatchNorm'd f32 lstm2 output of the window - and the same y
 * arrays; ONE sig f32 [rows][T][50] for both models - the normalised samples of the window's T events - because both read the
 * same samples.  A row is 512 T bytes per model and 200 T bytes shared; the depth's own cap is NRV_FIT_MAX_SIGNAL_ROWS
 * (environment, read by nrv_create; default 2^20); a call that would pass it is refused whole, by that name.
 *   nrv_fit_add_reads_raw  unchanged signature and label rule; the NRV_PREC_F32 kernels whatever the mode.  Where the lstm3 depth
 *     gathers, a gather moves every labelled window's T x 128 lstm2 values through the view the f32 lstm3 launch reads (16 bytes
 *     at a time) and its T x 50 samples out of the group's event-major samples (window w, step t is event w + t; 8 bytes at a
 *     time) to the window's slot, with plain stores.
 *   nrv_fit_set_rows_signal / nrv_fit_get_rows_signal  the unit doors.  Each depth's doors are refused at the other depths under
 *     their own names; the handle stays usable.
 * THE FIT.  One vector of NRV_FIT_PARAMS_SIGNAL(T, C) = 25896 + NRV_FIT_PARAMS_LSTM3(T, C) floats:
 *   [w1 24 | b1 8 | w2 192 | b2 8 | Ws 25600 | bs 64 | the lstm3 depth's vector]          tensors as the weight file has them.
 * params NULL: the handle's own tensors and zero centres.  Forward per (row, t): a1 = relu(conv1(sig) + b1), c1 = a1 s1 + h1,
 * a2 = relu(conv2(c1) + b2), F[p * 8 + o] = a2 s2 + h2 + sig[p] (`same` padding: taps outside the 50 samples are zero),
 * S = F Ws + bs, Xin = [x2 | S], then the lstm3 depth's forward and loss.  Backward: the lstm3 depth's, then dS = columns
 * 128 .. 191 of (sum over both directions, forward first, of dz3 W3^T), gWs = F^T dS, gbs = 1^T dS, dF = dS Ws^T, and back through
 * the two convolutions with the ReLU sides decided on the forward value (csrc/nrv_signalfit.h).  Chunks, reduction, finite check
 * over the whole vector and ONE Adam launch as at lstm3 depth; no atomics, the same calls give the same bytes.  nrv_fit_eval runs
 * the forward launches alone. */
#define NRV_FIT_SIGNAL 16
#define NRV_FIT_PARAMS_SIGNAL(T, C) (25896 + NRV_FIT_PARAMS_LSTM3(T, C))
int nrv_fit_set_rows_signal(nrv_handle* h, const float* x2_1, const float* x2_2, const float* sig, const uint8_t* y1, const uint8_t* y2,
                            int64_t n);
int nrv_fit_get_rows_signal(nrv_handle* h, int64_t first, int64_t count, float* x2_1, float* x2_2, float* sig, uint8_t* y1, uint8_t* y2);

/* ---- Fitting the read branch too - the whole model: the sixth and last DEPTH of nrv_fit_* (opt-in) ----
 * At depth NRV_FIT_FULL lstm1 - the 6 -> 16 Bi-LSTM on the read features, tensors 12 .. 17, 2944 weights - and lstm2 - the 32 -> 64
 * Bi-LSTM behind it, tensors 22 .. 27, 49664 weights - are fitted with everything the signal depth fits: every tensor of the 60
 * that is no BatchNorm's has a gradient on the device.  nanoreviser_amd/fullfit.py is the definition.  Frozen: the five
 * BatchNorms (2 .. 5, 8 .. 11, 18 .. 21, 28 .. 31, 40 .. 43).  THE STATED DEVIATIONS are the signal depth's, with bn_l1 and bn_l2
 * under the first: X1b = h1 * s_l1 + h_l1 and X2b = h2 * s_l2 + h_l2 from the moving statistics as the handle holds them (one f32
 * multiply and one f32 add), where Keras in training phase would normalise with the batch's statistics and fit gamma and beta;
 * Dropout is not applied while nrv_fit_set_dropout is off.  The constant is 32: 18 .. 31 and 33 are refused, and everything refused before stays refused.
 *   nrv_fit_set_depth  takes NRV_FIT_FULL under the rules above.
 * THE SET at this depth.  ONE sig f32 [rows][T][50] and ONE feat f32 [rows][T][6] for both models - the window's raw inputs, what
 * nrv_predict* takes; both models read the same - and the same y arrays: 224 T bytes per row.  The depth's own cap is
 * NRV_FIT_MAX_FULL_ROWS (environment, read by nrv_create; default 2^22, 10.3 GB at T = 11); a call that would pass it is refused
 * whole, by that name.
 *   nrv_fit_add_reads_raw  unchanged signature and label rule.  Nothing of the set depends on the network, so no launch group
 *     runs: behind the segmentation of a stage, one gather moves every labelled window's T x 50 samples and T x 6 features out of
 *     the stage's event-major arrays (window w, step t is event w + t; 8 bytes at a time) to the window's slot, with plain
 *     stores.  The set is the same bytes in every precision mode.
 *   nrv_fit_set_rows_full / nrv_fit_get_rows_full  the unit doors.  Each depth's doors are refused at the other depths under
 *     their own names; the handle stays usable.
 * THE FIT.  One vector of NRV_FIT_PARAMS_FULL(T, C) = 52608 + NRV_FIT_PARAMS_SIGNAL(T, C) floats:
 *   [W1f [6][64] | U1f [16][64] | b1f [64] | W1b | U1b | b1b | W2f [32][256] | U2f [64][256] | b2f [256] | W2b | U2b | b2b |
 *    the signal depth's vector]        kernels row-major [in][out], gate columns i, f, c, o, tensors as the weight file has them.
 * params NULL: the handle's own tensors as the file has them, no BatchNorm folded in, and zero centres.  Forward: lstm1 and lstm2
 * by the lstm3 depth's step rule (the backward direction walks t = T - 1 .. 0), Xin = [X2b | S], then the signal depth's forward
 * and loss.  Backward: the signal depth's, with ALL 192 columns of dXin = sum over both directions, forward first, of dz3 W3^T;
 * dH2 = dXin[.., :128] s_l2, back through time in lstm2, dH1 = (sum over both directions of dz2 W2^T) s_l1, back through time in
 * lstm1; gW = sum x_t^T dz, gU = sum h_{s-1}^T dz (bytes of zero at T = 1), gb = sum dz (csrc/nrv_fullfit.h).  Chunks, finite check
 * over the whole vector and ONE Adam launch as at signal depth; no atomics, the same calls give the same bytes.  nrv_fit_eval runs
 * the forward launches alone. */
#define NRV_FIT_FULL 32
#define NRV_FIT_PARAMS_FULL(T, C) (52608 + NRV_FIT_PARAMS_SIGNAL(T, C))
int nrv_fit_set_rows_full(nrv_handle* h, const float* sig, const float* feat, const uint8_t* y1, const uint8_t* y2, int64_t n);
int nrv_fit_get_rows_full(nrv_handle* h, int64_t first, int64_t count, float* sig, float* feat, uint8_t* y1, uint8_t* y2);

/* ---- Re-estimating the BatchNorm statistics inside the fitted section from rows of the set (opt-in) ----
 * nanoreviser_amd/bnfit.py is the definition.  The BatchNorms INSIDE the fitted section are, in tensor order: at depth
 * NRV_FIT_LSTM3 bn_l3 (tensors 40 .. 43); at NRV_FIT_SIGNAL bn_c1 (2 .. 5), bn_c2 (8 .. 11), bn_l3; at NRV_FIT_FULL also bn_l1
 * (18 .. 21) and bn_l2 (28 .. 31) between them; none at the other depths.  nrv_fit_begin at these three depths copies the
 * handle's folded (scale, shift) pairs into a block of the FIT's own, and every fit launch reads a BatchNorm there: without a
 * re-estimation every depth computes what it computed.  The handle's own model - nrv_predict*, the set's gathers - is never
 * changed: to run a re-estimated model, write it (bnfit.with_stats) and create a handle from it.
 *   nrv_fit_bn_reestimate  between nrv_fit_begin and the end of the fit, at any point, at the model's CURRENT parameters; Adam's
 *     state and the step counter are left alone.  Per channel of each BatchNorm, over the given rows (an index may repeat): the
 *     mean and the BIASED variance of the activation it normalises - bn_c1: a1 = relu(conv1(sig) + b1) over (row, t, the 50
 *     samples); bn_c2: a2 = relu(conv2(c1) + b2) likewise; bn_l1 / bn_l2 / bn_l3: the RAW Bi-LSTM output over (row, t).  With
 *     the pivot p = the LOADED moving mean: S1 = sum (x - p), S2 = sum (x - p)^2 in f64, m = S1 / N, mean = p + m,
 *     var = max(S2 / N - m m, 0), no contraction, each rounded once to f32.  Stages in dependency order - {bn_c1, bn_l1},
 *     {bn_c2, bn_l2}, {bn_l3} - one pass over the rows each (three at signal and full depth, one at lstm3 depth): behind a stage
 *     its new statistics are folded with the loaded gamma and beta exactly as nrv_create folds a file's tensors, and the next
 *     stage runs on them.  gamma and beta are never touched.  The forward launches are the fit's own, in its chunks
 *     (csrc/nrv_bnfit.h: the moments); no atomics, the same calls give the same bytes.  Refused under its own name, the handle
 *     staying usable: depths with no BatchNorm inside, no nrv_fit_begin for the model, n_rows <= 0, a row index outside the set,
 *     a raw-read call in flight.
 *   nrv_fit_bn_count  BatchNorms inside the section: 0, 1, 3 or 5.
 *   nrv_fit_bn_get    BatchNorm `which` of them: info (tensor_base: its gamma's tensor; n: elements per channel of the last
 *     re-estimation, 0 before any - then mean / var are the loaded statistics and s1 / s2 zero), mean, var [channels] f32,
 *     s1, s2 [channels] f64; any output may be NULL. */
typedef struct { int tensor_base; int channels; int64_t n; } nrv_fit_bn_info;
int nrv_fit_bn_reestimate(nrv_handle* h, int model, const uint32_t* rows, int64_t n_rows);
int nrv_fit_bn_count(nrv_handle* h);
int nrv_fit_bn_get(nrv_handle* h, int model, int which, nrv_fit_bn_info* info, float* mean, float* var, double* s1, double* s2);

/* ---- Fitting gamma and beta of the BatchNorms inside the fitted section (opt-in) ----
 * nanoreviser_amd/bnaffine.py is the definition.  A BatchNorm inside the section stays in its inference form on the CURRENT
 * moving statistics, y = x s + h with r = 1 / sqrt(var + 1e-3), s = gamma r, h = beta - mean s, folded in f32 exactly as
 * nrv_create folds a file's tensors; the statistics stay frozen during a step (Keras in training phase would normalise with the
 * batch's - that deviation remains) and move only by nrv_fit_bn_reestimate.  gamma and beta become parameters:
 *     g_gamma = r sum dy (x - mean) / b          g_beta = sum dy / b
 * per channel over (row, t) (and the 50 samples for a conv BatchNorm), dy the derivative of the batch's SUM of row losses by the
 * BatchNorm's output, x the activation it normalises; the sum is formed in the pivoted form, never as sum dy x - mean sum dy.
 * THE VECTOR.  While the switch is on, nrv_fit_begin, _grad, _epoch, _eval and _params take and return vectors with a block in
 * FRONT: for every BatchNorm inside, in tensor order, gamma [C] then beta [C] - NRV_FIT_PARAMS_BN(depth) floats.
 *   nrv_fit_set_bn_affine  on = 1 / 0.  May be called with rows in the set (the set does not depend on it); forgets any
 *     nrv_fit_begin of both models (the vector has another length).  nrv_fit_set_depth switches it off.  Refused under its own
 *     name, the handle staying usable: a raw-read call in flight; on = 1 at a depth with no BatchNorm inside (NRV_FIT_TAIL,
 *     NRV_FIT_HEAD, NRV_FIT_LSTM4).
 *   nrv_fit_bn_affine      1 while it is on, else 0.
 *   nrv_fit_begin          params = NULL starts the block from the handle's own gamma / beta; the pairs are folded ON THE DEVICE
 *     from the block and the handle's statistics and are the bytes nrv_create folded.
 *   a step                 the two sums leave the launch that holds the unscaled dy (csrc/nrv_bnaffine.h) as per-workgroup
 *     partials, added in ascending order by a reduce launch with a flag range of its own; the block takes part in the finite
 *     check over the whole vector and in the ONE Adam launch; behind the update one launch refolds (s, h) from the vector's
 *     gamma / beta and the block's current mean / variance.  No atomics; the same calls give the same bytes; nrv_fit_epoch
 *     still enqueues everything without a host synchronisation.
 *   nrv_fit_bn_reestimate  folds each stage with the vector's CURRENT gamma / beta; the pivot stays the loaded mean; gamma,
 *     beta, Adam's state and t keep their bytes, and later refolds use the new statistics.
 * To run a fitted model, write it (bnaffine.fitted_model) and create a handle from it. */
#define NRV_FIT_PARAMS_BN(depth) ((depth) == NRV_FIT_LSTM3 ? 512 : (depth) == NRV_FIT_SIGNAL ? 544 : (depth) == NRV_FIT_FULL ? 864 : 0)
int nrv_fit_set_bn_affine(nrv_handle* h, int on);
int nrv_fit_bn_affine(nrv_handle* h);

/* THE DROPOUT BEHIND THE IDENTITY BLOCK (opt-in; depths NRV_FIT_SIGNAL and NRV_FIT_FULL).  The reference model is identity block ->
 * Dropout(0.2) -> Flatten -> Dense(400 -> 64); F [pair][400] (f = p * 8 + o) is that Flatten's output.  While the switch is on,
 * nrv_fit_grad and nrv_fit_epoch drop F as Keras in training phase does; nanoreviser_amd/dropout.py is the definition.
 * THE RULE.  No generator with a state: the mask is a pure function of (seed, draw, model, set row, t, element).  Element f
 * belongs to quad q = f / 4; the four words of philox4x32_10(counter = (row, model << 16 | t * 100 + q, draw low, draw high),
 * key = (seed low, seed high)) serve f = 4 q .. 4 q + 3 in order; `row` is the row's index in the set, not its place in a batch or
 * a chunk; an element is kept iff its word >= thr = floor(rate * 2^32); keepf = (float)(1 - rate); forward Fd = F / keepf where
 * kept, else 0; backward dF = dFd / keepf where kept, else 0 - both correctly rounded divisions.  sig_dense's gradient multiplies
 * the dropped F.  `draw` counts batches and is a HOST counter per model.
 *   nrv_fit_set_dropout       rate in [0, 1), 0 = off (the default); resets both models' draws to 0; does NOT forget an
 *     nrv_fit_begin (the vector keeps its length).  nrv_fit_set_depth switches it off.  Refused under its own name, the handle
 *     staying usable: a rate outside [0, 1); rate > 0 at a depth whose signal branch is frozen; a raw-read call in flight;
 *     rate > 0 with T > 655 (t * 100 + q has 16 bits).
 *   nrv_fit_dropout           the getter: rate, seed and both models' draws; any output may be NULL.
 *   nrv_fit_set_dropout_draw  sets a model's draw (>= 0): what a continued run and the tests use.
 *   nrv_fit_dropout_mask      the unit door: uint8 [b][T][400], 1 = kept, for b set rows (any uint32; repeats allowed) at `draw`.
 *     Refused while the switch is off.
 *   nrv_fit_begin             resets that model's draw to 0.
 *   nrv_fit_grad              drops at the current draw and leaves it.
 *   nrv_fit_epoch             batch k of the call drops at draw + k; the draw then advances by ceil(n / B), skipped non-finite
 *     batches included; no host synchronisation inside an epoch.  The statistics are the dropped forward's, as Keras reports a
 *     training loss.
 *   nrv_fit_eval, nrv_fit_bn_reestimate   never drop.
 * With the switch off every launch is the instantiation it was and every depth returns the bytes it returned.  No atomics; the
 * same calls give the same bytes.  LEFT OUT: the draw is not persisted in a written model; dropout at depths whose signal
 * branch is frozen (there is nothing to drop); normalising with the batch's statistics. */
int nrv_fit_set_dropout(nrv_handle* h, double rate, uint64_t seed);
int nrv_fit_dropout(nrv_handle* h, double* rate, uint64_t* seed, int64_t draw[2]);
int nrv_fit_set_dropout_draw(nrv_handle* h, int model, int64_t draw);
int nrv_fit_dropout_mask(nrv_handle* h, int model, const uint32_t* rows, int b, int64_t draw, uint8_t* mask);

/* Same two calls with DEVICE pointers, enqueued on the handle's stream without a host sync
 * (call nrv_sync, or synchronise the stream you passed to nrv_set_stream).  The inputs must be
 * complete in stream order.  The handle's own stream is a blocking stream, i.e. it is ordered
 * after work already queued on the legacy default stream (where e.g. torch produces tensors by
 * default); producers on any other stream must be synchronised by the caller, or the handle
 * pointed at that stream with nrv_set_stream.
 * Alignment is C's: 4 bytes for the float arrays, 1 for d_a1 / d_a2; a pointer may lie anywhere inside an allocation.
 * No byte outside [n][T][50] / [n][T][6] in (read form: [N][50] / [N][6]) and [n][6], [n][5], [n], [n] out (read form:
 * n = N-T rows) is read into a result or written, whatever the launch grouping.
 * Each of d_p1, d_p2, d_a1, d_a2 may be NULL: that output is not produced, the others are unchanged by it. */
int nrv_predict_device(nrv_handle* h, const float* d_signal, const float* d_read, int64_t n,
                       float* d_p1, float* d_p2, int8_t* d_a1, int8_t* d_a2);
int nrv_predict_read_device(nrv_handle* h, const float* d_sig_ev, const float* d_feat_ev,
                            int64_t N, float* d_p1, float* d_p2, int8_t* d_a1, int8_t* d_a2);

/* Windows per launch group (Keras' predict(batch_size=...)); default 4096.  Results do not depend on the
 * grouping (every window is its own row of every kernel).  A group below 4096 windows would leave most of the
 * chip idle, so consecutive smaller groups of ONE call are coalesced into 4096-window launches (nrv_get_batch
 * still reports what was set); values above 4096 make larger launches (measured: no gain, the workspace
 * outgrows the Infinity Cache).  NRV_COALESCE=0 in the environment restores the uncoalesced form, in which
 * groups of <= 2048 windows (batch % 32 == 0) run concurrently on several streams. */
int nrv_set_batch(nrv_handle* h, int batch_windows);
int nrv_get_batch(nrv_handle* h);

/* Matrix arithmetic of the three large Bi-LSTM layers (32->64, 192->128, 256->64), the per-timestep
 * dense layers (128->128->32->6) and the signal branch's 400->64 layer: 98 % of the FLOPs.  All modes
 * accumulate in f32 and meet the same parity bars (every test of tests/test_gpu_parity.py runs once per
 * mode; DESIGN.md 5 has the figures over all 81 770 fixture windows: 0 argmax differences in any mode):
 *   NRV_PREC_F16X2 (default)  every operand is scaled by a power of two fixed at nrv_create from static
 *                    bounds, split into two f16 terms, and each product formed from three term pairs
 *                    on the f16 matrix pipe; activations travel between the kernels already split.
 *                    ~2.6x the f32 mode's throughput.
 *   NRV_PREC_BF16X3  every f32 operand is split exactly into three bf16 terms and each product formed
 *                    from the six term pairs that matter, on the bf16 matrix pipe; ~1.5x f32 mode;
 *   NRV_PREC_F32     plain f32 matrix instructions.
 * The convolutions, the first Bi-LSTM (6->16) and the per-window tail are f32 in every mode.
 * Range of NRV_PREC_F16X2: every activation has a static bound except the signal branch (the reference
 * normalises samples as (raw - median) / MAD without clipping, preprocessing.py:120-131, and computes in
 * f32, nanorevcnn.py:24-37, so spike samples and tiny MADs have a well-defined answer).  The f16x2 signal
 * branch represents |S| < 1023; a launch group that leaves that range (or carries a NaN / Inf sample)
 * is detected on the device and NEVER returned as is: see nrv_saturated.
 * Takes effect from the next call.  The environment variable NRV_PRECISION=f32|bf16x3|f16x2 sets the
 * mode a new handle starts in. */
#define NRV_PREC_F32 0
#define NRV_PREC_BF16X3 1
#define NRV_PREC_F16X2 2
int nrv_set_precision(nrv_handle* h, int mode);
int nrv_get_precision(nrv_handle* h);

/* Range guard of NRV_PREC_F16X2 (no-op in the other modes, which keep f32 buffers).
 *   Host-pointer entry points (nrv_predict, nrv_predict_read, nrv_predict_reads_raw): a pipeline stage whose
 *   signal branch left the f16 range is re-run on the NRV_PREC_F32 kernels before its results are handed over;
 *   *reruns counts such stages since nrv_create (informational - the results are already the f32 mode's).
 *   Device-pointer entry points (asynchronous): *pending is non-zero when a launch group enqueued since the
 *   previous nrv_saturated call left the range; the outputs of those calls must be discarded and the calls
 *   repeated after nrv_set_precision(h, NRV_PREC_F32) (engine.Reviser.predict_device_checked does that).
 *   Synchronises the handle's stream and clears the pending count.  Either pointer may be NULL. */
int nrv_saturated(nrv_handle* h, int64_t* pending, int64_t* reruns);

/* Use an existing hipStream_t (e.g. torch's current stream); NULL restores the handle's own. */
int nrv_set_stream(nrv_handle* h, void* hip_stream);
int nrv_sync(nrv_handle* h);

/* Per-kernel timing with HIP events recorded on the launch stream.  While enabled every
 * launch group is bracketed by events; nrv_prof_read synchronises, adds up the elapsed times
 * since the last read and returns, per kernel slot, total milliseconds and launch count.
 * Slots: 0 cnn, 1 lstm1, 2 lstm2, 3 lstm3, 4 lstm4, 5 head.  on = 1: every kernel (seven event
 * records per group, ~3 % of a 4096-window group); on = 2: only slot 3, the dominant kernel (two
 * records per group, ~12 us of idle pipe); on = 3: slot 3 on every 8th group only. */
#define NRV_N_KERNELS 6
int nrv_prof_enable(nrv_handle* h, int on);
int nrv_prof_read(nrv_handle* h, double* ms_total /*[NRV_N_KERNELS]*/,
                  int64_t* launches /*[NRV_N_KERNELS]*/);
const char* nrv_kernel_name(int slot);
/* Mean elapsed time, in microseconds, of an EMPTY bracket (two event records back to back on the handle's stream):
 * what a bracketed launch's figure contains beyond the kernel's own duration.  bench.py reports it next to the
 * bracketed figures so that they can be set against a rocprofv3 kernel trace of the same command. */
int nrv_prof_overhead(nrv_handle* h, double* us);

/* Message of the last failure on this handle (or, with h == NULL, of the last failed
 * nrv_create on this thread).  Never NULL. */
const char* nrv_last_error(nrv_handle* h);

/* Number of HIP devices visible to this process (0 when there is none or the runtime fails): what
 * the command line shards reads over (NanoReviser.py:214-219 sharded files over Pool workers). */
int nrv_device_count(void);

/* Always NRV_BACKEND_HIP: the library has no other backend. */
int nrv_backend(nrv_handle* h);

/* Window length the handle was created with. */
int nrv_window(nrv_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* NANOREV_H */
