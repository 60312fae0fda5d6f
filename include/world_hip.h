/* world_hip.h — C ABI of libworld_hip.so: the WORLD vocoder analysis/synthesis hot path as
 * hand-written HIP kernels for AMD MI355X (gfx950).
 *
 * The reference (tuanad121/Python-WORLD) has no FFI: its seam is the set of module-level stage
 * functions imported by world/main.py:14-23.  Each entry point below is the batched, device-side
 * replacement of ONE of those functions (cited per function); the Python mirror in
 * python-world_amd/world/ binds them with ctypes and keeps the reference's names, arguments and
 * result-dict keys.
 *
 * Conventions
 *  - every function returns 0 on success, non-zero on failure; wh_last_error() gives the text
 *    of the last failure on the calling thread.  No C++ exception crosses the boundary.
 *  - pointers named h_* are HOST pointers; all other data pointers are DEVICE pointers
 *    (hipMalloc / torch.cuda memory).  `stream` is a hipStream_t passed as void* (NULL = default).
 *    Calls are asynchronous with respect to the host unless stated.
 *  - dtype is IEEE float64 everywhere (the reference is float64 end to end).
 *  - a *batch* is a set of utterances concatenated sample-wise (x, offsets h_x_off[n_utt+1]) and
 *    frame-wise (per-frame arrays, offsets h_frame_off[n_utt+1]).  Utterances are independent.
 *  - dense per-frame outputs are FRAME-MAJOR on the device: spectrogram[frame][bin] (the
 *    reference's NumPy arrays are (bins, frames); the Python mirror transposes at the boundary).
 *  - nothing is retained past return except inside wh_ctx / wh_batch objects.
 */
#ifndef WORLD_HIP_H
#define WORLD_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct wh_ctx wh_ctx;     /* one per device per host thread: twiddle tables + scratch */
typedef struct wh_batch wh_batch; /* utterance/frame offsets of one batch, resident on the device */

int wh_version(void);
const char* wh_last_error(void);

/* ---- device / memory helpers (so a host without torch can drive the library) ------------- */
int wh_device_count(int* count);
int wh_ctx_create(int device, wh_ctx** out);
int wh_ctx_destroy(wh_ctx* ctx);
/* Free the context's scratch (workspace arena, per-call buffers: they only grow with the largest batch served); tables and
 * flags stay, the next call allocates again.  Synchronises the device.  A time base held by the context is dropped, and a
 * hipGraph captured over calls of this context holds the freed addresses: capture again instead of replaying it. */
int wh_ctx_trim(wh_ctx* ctx);
int wh_malloc(void** dptr, size_t bytes);
int wh_free(void* dptr);
int wh_memcpy_h2d(void* dst, const void* h_src, size_t bytes, void* stream);
int wh_memcpy_d2h(void* h_dst, const void* src, size_t bytes, void* stream);
int wh_memset(void* dst, int value, size_t bytes, void* stream);
int wh_stream_sync(void* stream);
/* Pinned, device-mapped host memory (hipHostMalloc): the GPU can read and write it through the same address. */
int wh_host_alloc(void** h_ptr, size_t bytes);
int wh_host_free(void* h_ptr);
/* Copy `bytes` (a multiple of 8) between two device-ACCESSIBLE pointers with a kernel on `stream`: either side may be
 * device memory or pinned host memory from wh_host_alloc / torch's pin_memory().  Unlike wh_memcpy_* this never
 * touches a DMA engine queue: an upload issued this way cannot be serialised behind a long download that another
 * stream has queued on the same engine (bench.py with_transfers_pipelined).  `max_blocks` <= 0 picks 64 workgroups
 * (enough to saturate PCIe, a quarter of the CUs at most). */
int wh_copy_mapped(wh_ctx* ctx, void* stream, void* dst, const void* src, size_t bytes, int max_blocks);

/* Sticky device-side condition flags raised by kernels instead of failing silently; reading them
 * synchronises the stream and clears them.  h_flags16[WH_FLAG_*] != 0 means the condition occurred. */
#define WH_FLAG_STONEMASK_WINDOW 0 /* a frame's f0 needed a longer window than kmax: left unrefined */
#define WH_FLAG_EVENT_OVERFLOW 1   /* a zero-crossing list exceeded its capacity (DIO: cannot happen, cap = len/2+2; Harvest: see wh_harvest_set_event_caps) */
#define WH_FLAG_NOISE_SHORT 2      /* synthesis ran out of host-supplied noise samples */
#define WH_FLAG_NO_PULSE 3         /* an utterance produced no pulse (reference asserts, synthesis.py:131) */
#define WH_FLAG_PULSE_OVERFLOW 4   /* more pulses than the pulse capacity, or more overlap-add rows than its row region holds */
#define WH_FLAG_OOB 5              /* bounds build only (wh_bounds_build() == 1): a kernel indexed outside a named buffer */
#define WH_FLAG_MLPG_PIVOT 6       /* wh_mlpg: a pivot of a system's LDL^T was not a positive finite number (non-finite or non-positive variances): that system's track is unspecified */
#define WH_FLAG_LSF 7              /* wh_lpc_levinson: a frame's r[0] was negative or not finite, or a prediction error on the way was not a positive finite number; wh_lsf_from_lpc: the finest grid still showed fewer than p/2 sign changes of a series — that frame's outputs are NaN */
int wh_take_flags(wh_ctx* ctx, void* stream, int32_t* h_flags16);
/* The bounds build of the library (tools/build_variants.py ...:-DWH_BOUNDS=1; a test vehicle, never the shipped file):
 * the covered kernels index their buffers through checked pointers (csrc/wh_device.h, wh::ckp); an access outside a
 * buffer is redirected to its first element, counted, and the first one recorded.  wh_take_flags then reports
 * WH_FLAG_OOB, and wh_bounds_last returns that record: out4 = {accesses out of range since the previous take, buffer
 * tag (WH_CK_* of wh_device.h), element index, elements in the buffer}.  In a normal build wh_bounds_build() is 0, the
 * flag is never set and the record is all zeros. */
int wh_bounds_build(void);
int wh_bounds_last(int64_t* out4);
/* Positive control (bounds build; fails elsewhere): a kernel that stores one element past a four-element checked
 * buffer — the next wh_take_flags must report WH_FLAG_OOB with the record {1, WH_CK_TABLE (7), 4, 4}. */
int wh_bounds_selftest(wh_ctx* ctx, void* stream);
/* Test hook: the spectral kernels' own log / exp / sincospi (csrc/wh_math.h: a few ulp, a third of the device library's
 * instructions) applied to a DEVICE array: which = 0 log -> out[n], 1 exp -> out[n], 2 (sin, cos)(pi x) -> out[2n];
 * which = 3, 4, 5: the same three in their table-driven forms (tlog, texp, tsincospi), the outputs laid out alike. */
int wh_math_probe(wh_ctx* ctx, void* stream, int which, const double* in, double* out, int64_t n);
/* Test hook (host only, no GPU): the table of the table-driven exp and log as it is uploaded (csrc/wh_math.h: layout).
 * h_out == NULL: returns the number of doubles; otherwise n_entries must be that number, and 0 is returned on success. */
int wh_math_table_read(double* h_out, int64_t n_entries);
/* Test hook: the wave-local FFT engine (wh::fft_lds_wave, csrc/wh_fft.h) on DEVICE data: `count` unnormalised complex
 * transforms of n = 512 points, interleaved (re, im) doubles, in -> out; inverse = 1: exp(+2 pi i k j / n), not divided by
 * n.  (gt, snt): threads per transform group and per workgroup, one of (64, 64), (128, 256), (256, 256). */
int wh_fft_probe(wh_ctx* ctx, void* stream, int n, int gt, int snt, int inverse, const double* in, double* out, int64_t count);
/* Test hook: the packed workgroup reductions of csrc/wh_reduce.h (block_sum2 | block_sum3 | block_sum5: k = 2 | 3 | 5) in one
 * workgroup of nt threads (64, 128, 256 or 512) on DEVICE data (csrc/wh_reduce_probe.hip).  in: k rows of nt doubles, value
 * k of thread t at in[k nt + t].  out: 2 k doubles per thread, out[t 2 k + j]: j < k the packed routine's total of value j as
 * thread t received it, j >= k the same total by one wave_sum per value and the waves added in ascending order from 0.0. */
int wh_reduce_probe(wh_ctx* ctx, void* stream, int nt, int k, const double* in, double* out);
/* Test hook: the workgroup-wide transforms of csrc/wh_fft.h on DEVICE data, at the shapes the kernels instantiate them
 * with (csrc/wh_fft_probe.hip lists them; any other shape fails with a message).  kind 0: fft_lds<n, inverse, nt, snt, maxr>,
 * n complex -> n complex; 1: fft_lds_from_regs<n, false, nt, maxr>, the same, the input read straight into the registers of
 * the first pass (x[q] = element tid + q nt); 2: rfft_lds<n, nt, snt, maxr>, n reals -> n / 2 + 1 complex; 3:
 * irfft_lds<n, nt, snt, maxr>, n / 2 + 1 complex -> n reals; 4: fft_lds_wave<n, inverse, nt, snt>, n complex -> n complex on
 * the first wave of each nt-thread group.  Complex values are interleaved (re, im) doubles, `count`
 * transforms lie back to back in `in` and `out`; nothing is normalised.  A workgroup has snt threads and snt / nt buffers,
 * one transform per nt-thread group, all advancing through the same barriers; the buffers of a half-filled last workgroup
 * are zero.  inverse: 0 or 1 for kinds 0 and 4, 0 for kinds 1 and 2, 1 for kind 3. */
int wh_fft_engine_probe(wh_ctx* ctx, void* stream, int kind, int n, int nt, int snt, int maxr, int inverse, const double* in,
                        double* out, int64_t count);
/* Test hook: the context's twiddle block (csrc/wh_device.h: the tables exp(-2 pi i k / n) at [n, 2n), n = 2 ... 32768, and the
 * FFT passes' [k][r] tables behind them) copied to HOST memory as (re, im) doubles.  h_out == NULL: returns the number of
 * entries; otherwise n_entries must be that number, and 0 is returned on success. */
int wh_twiddle_read(wh_ctx* ctx, double* h_out, int64_t n_entries);
/* Test hook: D4C's rank selection (sum_smallest, csrc/wh_d4c_select.h; the hook: csrc/wh_d4c_probe.hip) on DEVICE data, with the template arguments d4c_kernel of
 * transform length n (512 ... 8192) gives it.  `count` rows of K = n / 2 + 1 non-negative values, one workgroup each;
 * out[c] = (sum of the m smallest values of row c, sum of all K), 1 <= m <= K - 1.  layout 0 hands the values to the threads
 * as the band stage does (job i of thread t: bins t + i FT and n / 2 - (t + i FT)); layout 1 puts bin k on thread
 * (K - 1 - k) % FT, slots filled in the order of k. */
int wh_d4c_select_probe(wh_ctx* ctx, void* stream, int n, int layout, int m, const double* vals, double* out, int64_t count);
/* Test hook: the run-resident spectral helpers of csrc/wh_d4c_runs.h on DEVICE data (csrc/wh_d4c_probe.hip).  `count` half spectra of K = n / 2 + 1
 * bins in `in`, one workgroup each, K results each in `out`.  which 0: low_band_replica_runs<n> with f0[c] and reach =
 * reach_or_half[c]; which 1: fill_mirrored_runs<n> and the sliding band sum BandWindow::run of half-width reach_or_half[c]
 * Hz (not divided by the width; half-widths outside [0, fs] give zeros), f0 unused.  f0, reach_or_half: DEVICE arrays of
 * `count` doubles. */
int wh_d4c_runs_probe(wh_ctx* ctx, void* stream, int n, int which, double fs, const double* f0, const double* reach_or_half,
                      const double* in, double* out, int64_t count);
/* Test hook: the same two operations in their LDS forms (csrc/wh_spectral.h: low_band_replica<ft>; fill_mirrored<ft, n> and
 * BandWindow) at cheaptrick_kernel's (n, ft): (256 | 512 | 1024, 128), (2048 | 4096, 256).  Arguments as above. */
int wh_spectral_probe(wh_ctx* ctx, void* stream, int n, int ft, int which, double fs, const double* f0,
                      const double* reach_or_half, const double* in, double* out, int64_t count);
/* Test hook: Harvest's back end — hv_prune_kernel and the contour kernels (FixF0Contour, SmoothF0, the pick onto the frame
 * grid) — on candidate maps the CALLER supplies (csrc/wh_hv_probe.hip), through the launchers wh_harvest calls.  n_utt
 * utterances of h_nf1[u] >= 1 frames of 1 ms, concatenated; output frames h_frame_off[u] .. h_frame_off[u + 1] (at least one
 * each) at the times tp (seconds, DEVICE).  rf0 / rsc (DEVICE, pool_n doubles each): candidate frequencies and scores;
 * h_lst (HOST, one per 1 ms frame): (first pool slot << 8) | count, count <= 105 — a frame's candidates in the reference's
 * row order, an absent row being a zero.  keep (DEVICE, 4 uint32 per 1 ms frame): bit k = entry k of the frame's list
 * survives; mode 0 reads it, mode 1 runs the prune and writes it.  mode 2 runs the smoothing and the pick alone: `rows`
 * holds the step-4 contour in row 4 on entry, and rf0 / rsc / h_lst / keep are not used.  Out: f0_out / vuv_out (DEVICE, per
 * output frame); rows (DEVICE): per utterance six rows of nf1 doubles at 6 x (frames in front of it) — base, steps 1 to 4,
 * smoothed; h_nsec (HOST, [n_utt]) and h_secs (HOST, [n_utt][sec_cap][5]): step 3's sections as (first, last, extended
 * first, extended last, kept); more than sec_cap sections fail.  Waits for `stream`. */
int wh_harvest_contour_probe(wh_ctx* ctx, void* stream, int mode, int n_utt, const int64_t* h_nf1, const int64_t* h_frame_off,
                             const double* tp, const double* rf0, const double* rsc, int64_t pool_n, const int64_t* h_lst,
                             uint32_t* keep, double* f0_out, double* vuv_out, double* rows, int32_t* h_nsec, int32_t* h_secs,
                             int64_t sec_cap);
/* The same flags without a host wait, for callers that keep a pipeline of batches in flight:
 *   wh_flags_post — enqueue (one 16-lane kernel on `stream`) the publication of the flags raised by everything before
 *     it on the stream to a pinned host word per flag, and clear them on the device (discard != 0: clear them
 *     without publishing — for work whose results have been abandoned);
 *   wh_flags_poll — read, WITHOUT synchronising, the conditions published since the last poll / take (h_flags16[i] != 0).
 * A condition is therefore reported at the first poll after its post has executed — late, never lost; wh_take_flags
 * (which synchronises) also reports whatever has been posted and not yet polled. */
int wh_flags_post(wh_ctx* ctx, void* stream, int discard);
int wh_flags_poll(wh_ctx* ctx, int32_t* h_flags16);

/* Per-kernel timing: while enabled every kernel launch of this ctx is bracketed by a HIP event pair on
 * its launch stream.  wh_profile_collect synchronises the device and returns one record per launch in
 * launch order: names = '\n'-joined kernel names, ms[i] = elapsed milliseconds. Clears the record list. */
int wh_profile_enable(wh_ctx* ctx, int on);
int wh_profile_collect(wh_ctx* ctx, char* names, size_t names_bytes, float* ms, int max_records, int* n_records);

/* ---- batch descriptor --------------------------------------------------------------------- */
/* h_x_off[n_utt+1]: sample offsets into the concatenated waveform; h_frame_off[n_utt+1]: frame
 * offsets into the concatenated per-frame arrays.  Synchronous: the descriptor is complete on return (small H2D
 * copies and one kernel on the NULL stream, which is waited for — work in flight on non-blocking streams is not). */
int wh_batch_create(wh_ctx* ctx, int n_utt, const int64_t* h_x_off, const int64_t* h_frame_off, wh_batch** out);
int wh_batch_destroy(wh_batch* b);
/* Frame count of one utterance: int(1000*n/fs/frame_period + 1) — world/dio.py:28, world/harvest.py:46. */
int64_t wh_num_frames(int64_t n_samples, double fs, double frame_period_ms);

/* ---- CheapTrick: replaces cheaptrick()  (world/cheaptrick.py:9-39) ------------------------ */
/* x[total_samples]; tp/vuv[total_frames]; f0[total_frames] is IN/OUT: unvoiced frames and frames
 * below 3*fs/(fft_size-3) are overwritten with 500 Hz exactly as the reference mutates
 * source_object['f0'] (cheaptrick.py:26-27,32-33).  spectrogram[total_frames][fft_size/2+1];
 * ps_spectrogram (optional, may be NULL) [total_frames][fft_size] interleaved (re,im) =
 * the reference's 'ps spectrogram'.  fft_size must be a power of two in [256, 4096]. */
int wh_cheaptrick(wh_ctx* ctx, void* stream, const wh_batch* b, const double* x, const double* tp, double* f0,
                  const double* vuv, double fs, int fft_size, double q1, double* spectrogram, double* ps_spectrogram);

/* ---- D4C: replaces d4c()  (world/d4c.py:10-64) ------------------------------------------------ */
/* f0 is IN/OUT: frames with vuv==0 are zeroed like the reference does (d4c.py:32).  The D4C FFT
 * size 2^ceil(log2(4fs/47+1)), the love-train FFT size and the band layout follow the reference.
 * aperiodicity[total_frames][fft_size_for_spectrum/2+1] (amplitude, 1-1e-12 on unvoiced frames);
 * coarse_ap (optional, may be NULL) [total_frames][wh_d4c_bands(fs,0)] = the reference's
 * 'coarse_ap' debug rows (negative dB). */
int wh_d4c(wh_ctx* ctx, void* stream, const wh_batch* b, const double* x, const double* tp, double* f0,
           const double* vuv, double fs, double threshold, int fft_size_for_spectrum, double* aperiodicity,
           double* coarse_ap);
/* Number of aperiodicity bands: floor(min(15000, fs/2-interval)/interval) (d4c.py:34, d4cRequiem.py:19). */
int wh_d4c_bands(double fs, int requiem);

/* ---- Band aperiodicity -> dense aperiodicity: the last step of d4c()  (world/d4c.py:45-59) -------- */
/* The expansion of a stored band aperiodicity (the reference's 'coarse_ap') into the dense rows that wh_synthesis
 * reads, without running D4C again:
 *   out[f][k] = 1 - 1e-12                                                                     where gate[f] == 0 (d4c.py:50)
 *             = 10 ** (interp(coarse_axis, [-60, coarse[f][:], -1e-12])(k * fs / fft_size) / 20)   otherwise (d4c.py:58-59)
 * with coarse_axis = [0, fi, 2 fi, ..., nap fi, fs / 2] (d4c.py:45), fi = frequency_interval in Hz, fft_size =
 * 2 (k_bins - 1).  coarse[n_frames][nap] holds the values as wh_d4c's coarse_ap does (negated dB; a -0.0 stays one),
 * gate[n_frames] is 0 for the frames D4C's voicing gate rejected (unvoiced ones among them) and non-zero for the others,
 * out[n_frames][k_bins].  All DEVICE pointers.  The rows are bit for bit the ones wh_d4c writes for the same frames: both
 * kernels evaluate the interpolation through the same device functions.  1 <= nap <= 8, nap * fi < fs / 2. */
int wh_aperiodicity_from_bands(wh_ctx* ctx, void* stream, int64_t n_frames, int nap, int k_bins, double fs,
                               int frequency_interval, const double* coarse, const double* gate, double* out);
/* gate[f] = 0.0 where row f of wh_d4c's aperiodicity[n_frames][k_bins] is the rejected frame's constant row, 1.0 where it
 * came from the bands: read from bin 0, which holds 1 - 1e-12 in the first case and 10^(-60/20) in the second. */
int wh_aperiodicity_gate(wh_ctx* ctx, void* stream, int64_t n_frames, int k_bins, const double* aperiodicity,
                         double* gate);

/* ---- D4C-Requiem: replaces d4cRequiem()  (world/d4cRequiem.py:9-44) ------------------------- */
/* fft_size <= 0 selects the reference default 2^ceil(log2(3fs/47+1)).
 * band_aperiodicity[total_frames][wh_d4c_bands(fs,1)+2] in dB (row 0 = -60, last = -1e-12). */
int wh_d4c_requiem(wh_ctx* ctx, void* stream, const wh_batch* b, const double* x, const double* tp, double* f0,
                   const double* vuv, double fs, double threshold, int fft_size, double* band_aperiodicity);

/* ---- DIO: replaces dio()  (world/dio.py:10-55) -------------------------------------------------- */
/* tp[total_frames]: frame times (s) = arange(nf)*frame_period/1000, nf = wh_num_frames(n, fs, frame_period).
 * The band filters are DATA supplied by the host (so that the even-length Nuttall argmax tie that fixes
 * each band's delay, dio.py:130-131, is decided by the host's NumPy exactly like the reference):
 *   h_band_f0[n_bands]   boundary f0 of each band: f0_floor*2^((i+1)/channels_in_octave)   (dio.py:32-34)
 *   h_band_len[n_bands]  tap count 4*int(target_fs/f/2+0.5);  h_band_taps: the Nuttall windows, concatenated
 *   h_band_bias[n_bands] argmax of each window (the reference's index_bias)
 *   h_lowcut[2*lowcut_half+1]  the zero-phase low-cut FIR of dio.py:80-83, lowcut_half = int(target_fs/50+0.5)
 * Outputs: f0_out, vuv_out [total_frames]; optional cand_out / raw_out: for utterance u a row-major
 * [n_bands][nf_u] block at offset frame_off[u]*n_bands (the reference's 'f0_candidates' / 'raw_f0_candidates').
 * Decimation ratio is int(fs/target_fs) and the decimated rate is taken as target_fs, like the reference. */
int wh_dio(wh_ctx* ctx, void* stream, const wh_batch* b, const double* x, const double* tp, double fs, double f0_floor,
           double f0_ceil, double target_fs, double frame_period_ms, double allowed_range, int n_bands,
           const double* h_band_f0, const int32_t* h_band_bias, const int32_t* h_band_len, const double* h_band_taps,
           const double* h_lowcut, int lowcut_half, double* f0_out, double* vuv_out, double* cand_out, double* raw_out);

/* ---- Harvest: replaces harvest()  (world/harvest.py:17-54) ---------------------------------------- */
/* tp[total_frames]: output frame times (s).  Host-supplied filter DATA (the reference obtains them from
 * SciPy / NumPy at run time, so the host language evaluates the same expressions):
 *   decimation_ratio r = int(fs/8000 + 0.5) (1 for fs <= 8000); if fs > 8000 — ALSO where r rounds to 1, 8 kHz < fs <
 *   12 kHz: harvest.py:60 branches on the rate and still low-pass filters — h_ba[8] = (b0..b3, a0..a3) of
 *   scipy.signal.cheby1(3, 0.05, 0.8/r) and h_zi[3] = scipy.signal.lfilter_zi(b, a)   (harvest.py:599-603); else
 *   h_ba = NULL or all zeros (a0 == 0: no filter);
 *   h_band_f0[n_bands]: channel centre frequencies (harvest.py:22-29, 152 for the default range);
 *   h_band_half[n_bands]: h = round-half-up(2*fs_d/f) (harvest.py:253);
 *   h_band_taps: concatenated band-pass FIRs nuttall(2h+1)*cos(2*pi*f*k/fs_d), k=-h..h (harvest.py:254-256).
 * Outputs f0_out / vuv_out [total_frames].  Optional debug outputs (DEVICE, may be NULL): dbg_y — the
 * decimated, mean-removed signals concatenated; dbg_raw — per utterance [n_bands][nf1] raw channel candidates
 * on the 1 ms grid; dbg_f0_1ms — the 1 ms contour before smoothing. */
int wh_harvest(wh_ctx* ctx, void* stream, const wh_batch* b, const double* x, const double* tp, double fs,
               double f0_floor, double f0_ceil, double frame_period_ms, int decimation_ratio, const double* h_ba,
               const double* h_zi, int n_bands, const double* h_band_f0, const int32_t* h_band_half,
               const double* h_band_taps, double* f0_out, double* vuv_out, double* dbg_y, double* dbg_raw,
               double* dbg_f0_1ms);
/* Capacities of Harvest's zero-crossing lists.  The reference keeps the four crossing trains of a channel as NumPy arrays
 * of whatever length they turn out to have (ZeroCrossingEngine, world/harvest.py:283-297); wh_harvest sizes its lists
 * from an estimate (three times the channel's centre frequency per second) before anything has run.  The estimate fails
 * where a stretch of the filtered signal is constant up to rounding — digital silence next to signal: harvest.py:69
 * removes the mean, the silence becomes a DC level, and the first difference of its filtered image changes sign at
 * random, as it does in the reference's own arithmetic.  Such a call raises WH_FLAG_EVENT_OVERFLOW and its results
 * are not to be used; its COUNTS are exact (counting goes on past a full list):
 *   wh_harvest_event_counts — h_caps_out[u * n_bands + i] (HOST) = the longest of the four trains of channel i of
 *     utterance u in this context's last wh_harvest; n = utterances x channels of that call.  Waits for `stream`.
 *   wh_harvest_set_event_caps — h_caps != NULL: these capacities for the NEXT wh_harvest of this context (one call);
 *     NULL, n == -1: the bound no signal exceeds (ylen/2 + 2 per train: 4.3 x the estimate's memory for the default
 *     range) for every later call; NULL, n == 0: back to the estimate.
 * A repeat with the counted capacities fits by construction (same arithmetic, same counts). */
int wh_harvest_set_event_caps(wh_ctx* ctx, const int64_t* h_caps, int64_t n);
int wh_harvest_event_counts(wh_ctx* ctx, void* stream, int64_t* h_caps_out, int64_t n);

/* ---- StoneMask: replaces stonemask()  (world/stonemask.py:8-27) -------------------------------- */
/* f0[total_frames] in, refined_f0[total_frames] out (a different buffer: the reference returns a new
 * array).  h_qtime[2*kmax+1] (HOST): h_qtime[k+kmax] = float("%.4f" % (k/fs)) — the reference
 * quantises its window time base through string formatting (stonemask.py:38); the table is built by
 * the host language so that the decimal rounding is exactly Python's.  kmax >= ceil(1.5*fs/min f0). */
int wh_stonemask(wh_ctx* ctx, void* stream, const wh_batch* b, const double* x, const double* tp, const double* f0,
                 double fs, const double* h_qtime, int kmax, double* refined_f0);

/* ---- Synthesis: replaces synthesis()  (world/synthesis.py:21-82) ------------------------------- */
/* Inputs per frame (batch frame layout): tp, f0, vuv [total_frames]; spectrogram and aperiodicity
 * [total_frames][fft_size/2+1] frame-major (aperiodicity = amplitude as produced by wh_d4c).
 * Output y: concatenated waveforms, offsets h_y_off[n_utt+1] (HOST).  The length of utterance u must be
 * len(np.arange(tp[0], tp[-1]+1/fs, 1/fs)) and its time axis is t_i = h_t0[u] + i*h_dt[u] with
 * h_dt = (t0 + 1/fs) - t0: NumPy's float arange semantics are evaluated by the host (synthesis.py:39; the
 * 48 kHz case yields 480002 samples, not 480001).
 * pulse_cap: pulse slots per utterance (>= number of pulses; ny/8+64 suffices for mean f0 < fs/8);
 *   overflow raises WH_FLAG_PULSE_OVERFLOW.
 * noise: optional DEVICE array of standard-normal samples, utterance u reads noise[h_noise_off[u] ..
 *   h_noise_off[u+1]); pulse i consumes max(3, noise_size_i) consecutive samples in pulse order — exactly
 *   the reference's np.random.randn call sequence (synthesis.py:93), so feeding np.random.randn(total)
 *   reproduces the reference bit-for-bit in the noise it uses.  noise == NULL: a counter-based Philox
 *   generator seeded by `seed` is used on the device instead (statistically equivalent, not the same samples).
 * pulse_count_out: optional DEVICE int32[n_utt]. */
int wh_synthesis(wh_ctx* ctx, void* stream, const wh_batch* b, const double* tp, const double* f0, const double* vuv,
                 const double* spectrogram, const double* aperiodicity, double fs, int fft_size, const int64_t* h_y_off,
                 const double* h_t0, const double* h_dt, int64_t pulse_cap, const double* noise,
                 const int64_t* h_noise_off, uint64_t seed, double* y, int32_t* pulse_count_out);
/* wh_synthesis in two halves, so that the half that depends on the time base alone can run early, on another stream:
 *   wh_synthesis_timebase — phase increments, the exact cumulative phase (np.cumsum, bit for bit), pulse positions and
 *     fractional shifts, noise offsets, per-pulse frame pairs (synthesis.py:118-152).  Inputs tp / f0 / vuv only.  The
 *     results stay in ctx's workspace until another call of that context uses the workspace.  f0_low_limit > 0: f0 is
 *     the F0 stage's output and is read as World.encode leaves it after CheapTrick and D4C (vuv == 0 -> 0, f0 <
 *     f0_low_limit = 3 fs / (fft_size - 3) -> 500 Hz), i.e. the call can be issued before those two stages have run.
 *   wh_synthesis_render — the spectral half: one response per pulse of the time base held by timebase_ctx (the same
 *     context or another one of the same device), overlap-added into y.  The caller orders it behind the time base
 *     (same stream, or an event wait).  Fails if timebase_ctx holds no time base for this batch / pulse_cap.
 * wh_synthesis(ctx, ...) == wh_synthesis_timebase(ctx, ..., 0) followed by wh_synthesis_render(ctx, ..., ctx, ...). */
int wh_synthesis_timebase(wh_ctx* ctx, void* stream, const wh_batch* b, const double* tp, const double* f0,
                          const double* vuv, double fs, const int64_t* h_y_off, const double* h_t0, const double* h_dt,
                          int64_t pulse_cap, double f0_low_limit);
int wh_synthesis_render(wh_ctx* ctx, void* stream, const wh_batch* b, const wh_ctx* timebase_ctx, const double* tp,
                        const double* spectrogram, const double* aperiodicity, double fs, int fft_size,
                        const int64_t* h_y_off, const double* h_t0, const double* h_dt, int64_t pulse_cap,
                        const double* noise, const int64_t* h_noise_off, uint64_t seed, double* y,
                        int32_t* pulse_count_out);
/* Pulse bookkeeping only (synchronous): per-utterance pulse count and the exact number of normal
 * samples the reference would draw, sum_i max(3, noise_size_i).  HOST outputs. */
int wh_synthesis_plan(wh_ctx* ctx, void* stream, const wh_batch* b, const double* tp, const double* f0,
                      const double* vuv, double fs, const int64_t* h_y_off, const double* h_t0, const double* h_dt,
                      int64_t pulse_cap, int32_t* h_pulse_count, int64_t* h_noise_total);
/* Test hook (read-only, no kernel): what the last wh_synthesis_timebase of ctx (also the one inside wh_synthesis) left
 * in its workspace, copied to HOST arrays so that every pulse can be compared with the reference's field by field.
 * Fails with "no time base" unless ctx holds one (any call that lays the workspace out again drops it), and when
 * n_utt, pulse_cap or n_samples are not that time base's.  Waits for `stream`.  Any output may be NULL.
 *   h_count[n_utt]: pulses per utterance (clipped to pulse_cap); h_base[n_utt + 1]: their exclusive prefix (p_base).
 *   Per pulse, n_utt * pulse_cap entries each of which the first h_base[n_utt] are written, utterance by utterance in
 *   time order: h_pidx (1-based sample index), h_time (pulse_locations), h_shift, h_noff (offset into the utterance's
 *   noise stream), h_noise_size (next index - this one, 0 for the last), h_vuv, h_row_lo / h_row_hi (the two frames the
 *   pulse interpolates between, relative to the utterance's first frame), h_weight (of the later frame; -1: one frame).
 *   Per output sample, n_samples entries: h_phase (cumulative phase), h_vuv_s (interpolated vuv > 0.5). */
int wh_synthesis_timebase_read(wh_ctx* ctx, void* stream, int n_utt, int64_t pulse_cap, int64_t n_samples,
                               int32_t* h_count, int64_t* h_base, int64_t* h_pidx, double* h_time, double* h_shift,
                               int64_t* h_noff, int32_t* h_noise_size, int32_t* h_vuv, int64_t* h_row_lo,
                               int64_t* h_row_hi, double* h_weight, double* h_phase, uint8_t* h_vuv_s);

/* The device noise of wh_synthesis / wh_synthesis_render (noise == NULL), exposed for sample-exact checks: out[i]
 * (DEVICE, n doubles) = sample q0 + i of the standard-normal stream that utterance `utt` of a batch reads under
 * `seed` — the stand-in for the reference's np.random.randn draws (world/synthesis.py:93): pulse i consumes samples
 * noff_i .. noff_i + max(3, noise_size_i) of it, exactly as it would consume a host-supplied `noise` stream, so a
 * decode with noise = this dump equals the decode with noise == NULL and the same seed. */
int wh_philox_normals(wh_ctx* ctx, void* stream, uint64_t seed, int utt, int64_t q0, int64_t n, double* out);

/* decode()'s peak normalisation (world/main.py:209-212): per utterance u, y[h_y_off[u] .. h_y_off[u+1]) is divided
 * by max|y| when that exceeds 1.  In place, on the stream; the workspace of ctx is used (call it after wh_synthesis*
 * has finished enqueueing, as the Python mirror does). */
int wh_peak_normalise(wh_ctx* ctx, void* stream, double* y, const int64_t* h_y_off, int n_utt);

/* The phase accumulator of synthesis() is np.cumsum over the per-sample phase increments (world/synthesis.py:128):
 * a sequential float64 sum whose rounding decides the pulse positions.  This entry exposes the routine that
 * reproduces it bit for bit (in place, n_seg independent segments of NON-NEGATIVE doubles, h_off[n_seg + 1] element
 * offsets into d_data) so that the agreement can be tested directly. */
int wh_cumsum_exact(wh_ctx* ctx, void* stream, double* d_data, const int64_t* h_off, int n_seg);

/* ---- Requiem synthesis: replaces synthesisRequiem()  (world/synthesisRequiem.py:12-25) ------------ */
/* band_aperiodicity[total_frames][n_bands] in dB as produced by wh_d4c_requiem (n_bands = bands+2 <= 8).
 * Seed tables (DEVICE, row-major like the reference's NumPy arrays): pulse_seed[pulse_fft][n_bands],
 * noise_seed[noise_len][n_bands] — built by the host (get_seeds_signals, world/get_seeds_signals.py:8).
 * h_hop[u] = int((tp[1]-tp[0])*fs) of utterance u (synthesisRequiem.py:78, truncating).
 * h_cursor[n_utt][n_bands]: read position in the circular noise seed at which utterance u starts — the
 * reference keeps this in a function attribute that persists across calls (synthesisRequiem.py:131-141);
 * after an utterance of ny samples the position is (cursor + ny - 1) mod noise_len.
 * y / h_y_off / h_t0 / h_dt / pulse_cap as for wh_synthesis. */
int wh_synthesis_requiem(wh_ctx* ctx, void* stream, const wh_batch* b, const double* tp, const double* f0,
                         const double* vuv, const double* spectrogram, const double* band_aperiodicity, double fs,
                         int fft_size, const int64_t* h_y_off, const double* h_t0, const double* h_dt, const int64_t* h_hop,
                         int64_t pulse_cap, const double* pulse_seed, int pulse_fft, const double* noise_seed,
                         int64_t noise_len, int n_bands, const int64_t* h_cursor, double* y);

/* ---- Spectral feature heads: replace World.encode_lfbank / encode_mcep / decode_mcep  (world/main.py:305-358) ---- */
/* One dense product per frame with an elementwise prologue and epilogue, on the FP64 matrix cores:
 *     out[f][n] = epi( sum_{k<ka} pro(a[f*lda + k], k) * h_w[k*nw + n] ),   f < n_rows, n < nw;  out row stride ldo
 *   prologue 0: pro(v) = v;  1: pro(v, k) = pscale * (v * h_p[k])^2  (encode_lfbank: pre-emphasis |H(k)| and
 *   1/nfft power, main.py:313-316);  2: pro(v) = log(v)  (encode_mcep, main.py:333)
 *   epilogue 0: none;  1: log with 0 -> DBL_EPSILON (main.py:321-322);  2: exp (decode_mcep, main.py:358);
 *   3: sqrt(max(0, v)) (SWIPE' loudness, swipe.py:42-44)
 * a / out: DEVICE, frame-major (wh_cheaptrick's spectrogram layout).  h_w[ka][nw] and h_p[ka] are HOST tables: the mel
 * filterbank transposed (get_filterbanks, main.py:275-303), or the cosine rows of the inverse / forward real FFT with
 * the mel warp of main.py:335-337 / 351-356 folded in — built by the host with the reference's own expressions. */
int wh_feature_matmul(wh_ctx* ctx, void* stream, const double* a, int64_t n_rows, int ka, int64_t lda, int prologue,
                      const double* h_p, double pscale, const double* h_w, int nw, int epilogue, double* out, int64_t ldo);
/* The same product with the weight table identified by the caller: `table_tag` != 0 promises that every call with this
 * tag (and the same ka x nw) passes the same h_w content.  The padded matrix is then built and uploaded on the first
 * call only and every later call is a look-up — no re-padding, no comparison of the host bytes (7 MB per SWIPE' call
 * at 16 kHz otherwise).  Tables of different content MUST carry different tags; table_tag == 0 is wh_feature_matmul. */
int wh_feature_matmul_tagged(wh_ctx* ctx, void* stream, const double* a, int64_t n_rows, int ka, int64_t lda, int prologue,
                             const double* h_p, double pscale, const double* h_w, int nw, int epilogue, double* out,
                             int64_t ldo, uint64_t table_tag);
/* get_context (main.py:360-365): out[i][j*d + c] = x[clamp(i + j - w, 0, n_rows-1)][c], j = 0..2w.  DEVICE pointers. */
int wh_context_frames(wh_ctx* ctx, void* stream, const double* x, int64_t n_rows, int d, int w, double* out);

/* ---- Manifold vocoder: the Dense stacks of World.encode_vae  (world/main.py:367-384) ------------------------------- */
/* One launch runs n_layers Dense layers (y = act(x W + b)) over n_rows rows; the activations stay on chip.
 *   x (DEVICE, frame-major, row stride ldx >= d): the input rows.  The first layer sees row i as get_context does
 *     (main.py:360-365): columns j*d + c = x[clamp(i + j - window)][c] - h_in_shift[c], j = 0..2 window, with the clamp
 *     to the row's own segment [h_seg_off[u], h_seg_off[u+1]) (HOST, int64, n_seg + 1 entries from 0 to n_rows), so that
 *     context never crosses an utterance.  h_in_shift (HOST, d doubles) may be NULL: no shift.  (2 window + 1) d <= 2048.
 *   h_units[l], h_act[l] (HOST): layer widths (<= 256 except the last) and activations, 0 linear, 1 relu, 2 tanh,
 *     3 sigmoid.  h_w (HOST): the layers' kernels [in_l][units_l] row-major, one after the other (in_0 = (2 window + 1) d,
 *     in_l = units_{l-1}); h_b (HOST): their biases.  Non-finite values are refused.
 *   The last layer computes only its columns [out_col0, out_col0 + n_out) (n_out <= 256), adds h_out_shift[n_out] (HOST,
 *     may be NULL) and writes out[i*ldo + n] (DEVICE).  tap_layer in [0, n_layers - 1) also writes that layer's output to
 *     tap_out[i*ld_tap + n] (DEVICE); tap_layer < 0: none.  tap_f32 != 0 rounds the tap layer's output to float32, in
 *     tap_out and as the next layer's input (Keras' encoder.predict hands the decoder a float32 latent).
 *   Every row's result is independent of the other rows of the launch.  table_tag != 0 promises that every call with
 *   this tag (and the same shapes) passes the same h_w / h_b: the padded FP64 copy is then uploaded once and looked up. */
int wh_dense_stack(wh_ctx* ctx, void* stream, const double* x, int64_t n_rows, int d, int64_t ldx, const int64_t* h_seg_off,
                   int n_seg, int window, const double* h_in_shift, int n_layers, const int* h_units, const int* h_act,
                   const double* h_w, const double* h_b, int out_col0, int n_out, int tap_layer, double* tap_out,
                   int64_t ld_tap, int tap_f32, const double* h_out_shift, double* out, int64_t ldo, uint64_t table_tag);

/* ---- SWIPE': replaces swipe()  (world/swipe.py:9-105; f0_method='swipe', world/main.py:45-46,134-135) ---------- */
/* One entry of the window-size table (HOST): candidates [j0, j0+n_c) of the candidate set use window size ws with
 * hop `hop` (= ws - noverlap of the reference's specgram call, swipe.py:35-38). */
typedef struct wh_swipe_window {
  int32_t ws, hop;          /* window length (power of two in [64, 16384]), hop in samples */
  int32_t j0, n_c;
  const double* h_window;   /* [ws]               np.hanning(ws + 2)[1:-1] */
  const double* h_interp;   /* [ws/2+1][n_erb]    magnitude bins -> ERB grid: interp1d(kind='cubic') as a matrix, k-major */
  const double* h_kernels;  /* [n_erb][n_c]       candidate kernels (pitchStrengthOneCandidate, swipe.py:127-146), k-major */
  const double* h_mu;       /* [n_c]              window-size membership weights (swipe.py:62-66) */
  uint64_t table_tag;       /* != 0: identity of (h_interp, h_kernels) for wh_feature_matmul_tagged (content-stable per tag) */
} wh_swipe_window;
/* x: concatenated waveforms (DEVICE); the batch's frame grid is the output grid t = arange(nf) * dt with
 * nf = int(1000*n/fs/(dt*1000) + 1).  HOST tables: h_pc[n_cand] candidate pitches, h_win[n_win], and for the parabolic
 * refinement of a maximum at candidate j (swipe.py:83-100): h_ntc[j][3] = normalised periods of candidates j-1..j+1,
 * h_fine[j][fine_stride] / h_n_fine[j] = the 1/768-octave evaluation grid (fine_stride must be 20).
 * s_thr: pitch-strength threshold (frames below it are unvoiced, f0 = 0).  Outputs f0_out / vuv_out [total_frames]. */
int wh_swipe(wh_ctx* ctx, void* stream, const wh_batch* b, const double* x, double fs, double dt, double s_thr, int n_cand,
             const double* h_pc, int n_erb, int n_win, const wh_swipe_window* h_win, const double* h_ntc,
             const double* h_fine, const int32_t* h_n_fine, int fine_stride, double* f0_out, double* vuv_out);

/* ---- Requiem seed signals on the device: replaces get_seeds_signals()  (world/get_seeds_signals.py:8-73) --------- */
/* pulse_seed[fft_size][n_bands] (DEVICE): the band pulses, deterministic, equal to the reference's up to rounding.
 * noise_seed[noise_length][n_bands] (DEVICE): modified velvet noise (segments of the reference's three short periods
 * chosen at random, one +-2 impulse per 4-sample cell at a random offset, signs balanced per segment in random
 * order) circularly convolved with each band pulse.  The randomness comes from a Philox-4x32-10 stream keyed by
 * `seed` instead of Python's `random` / NumPy's global generator: same construction and statistics, not the same
 * samples.  velvet_out (optional, may be NULL): the velvet noise itself [noise_length].
 * n_bands = wh_d4c_bands(fs, 1) + 2; fft_size / noise_length: the reference defaults are
 * 1024 * 2^ceil(log2(fs/48000)) and 2^ceil(log2(fs/2)). */
int wh_requiem_seeds(wh_ctx* ctx, void* stream, double fs, int fft_size, int64_t noise_length, int n_bands, uint64_t seed,
                     double* pulse_seed, double* noise_seed, double* velvet_out);

/* ---- Modifiers on a resident encoding: replace World.warp_spectrum / modify_duration  (world/main.py:180-196) ---- */
/* warp_spectrum: spectrogram[n_frames][k_bins] (DEVICE, in place): frame <- np.interp((k/K)^factor, k/K, frame).  The
 * query points are the same for every frame, so the host runs NumPy's search once per bin and passes (HOST tables)
 * h_src[k] = interval index j, h_dx[k] = x_k - xp[j], h_den[k] = xp[j+1] - xp[j], with h_den[k] = 0 where np.interp
 * returns fp[j] itself (exact knot / last knot / beyond it); the kernel applies NumPy's
 * (fp[j+1]-fp[j]) / den * dx + fp[j]. */
int wh_warp_spectrum(wh_ctx* ctx, void* stream, double* spectrogram, int64_t n_frames, int k_bins, const int32_t* h_src,
                     const double* h_dx, const double* h_den);
/* modify_duration: tp_out[f] = np.interp(tp_in[f], xp_u, fp_u) for the utterance u of frame f; h_xp / h_fp
 * [n_utt][n_anchor] (HOST): xp_u = [0, from_time..., last frame time of u], fp_u = to_time with a trailing -1 replaced
 * by that last frame time (main.py:186-189).  tp_out must not alias tp_in (the reference installs a new array). */
int wh_modify_duration(wh_ctx* ctx, void* stream, const wh_batch* b, const double* tp_in, double* tp_out,
                       const double* h_xp, const double* h_fp, int n_anchor);

/* ---- Pitch from outside and another frame grid: what World.set_pitch leaves open  (world/main.py:164-168) ----------- */
/* The reference's set_pitch raises NotImplementedError with the note that the values have to be resampled onto the frame
 * times the spectrogram shares.  These two entries do that resampling with np.interp's own arithmetic, bit for bit:
 * j = last knot with xp[j] <= x; fp[j] itself on an exact hit, at the last knot and beyond either end (the end values);
 * otherwise slope = (fp[j+1]-fp[j]) / (xp[j+1]-xp[j]) and slope*(x-xp[j]) + fp[j], unfused — and, as NumPy does, where
 * that is NaN slope*(x-xp[j+1]) + fp[j+1], and fp[j] where that is NaN too and fp[j] == fp[j+1].
 *
 * interp_contour: out[f] = np.interp(tp[f], time_u, value_u) for the utterance u of frame f.  The knot lists are ragged:
 * utterance u owns h_time / h_value[h_knot_off[u] .. h_knot_off[u+1]) (HOST; h_knot_off[n_utt+1] starts at 0; every
 * list holds at least one knot; times finite and strictly increasing, or the call fails before anything is launched).
 * voiced_rule != 0 (WORLD contours hold 0 at unvoiced frames; a straight line from 0 Hz to 200 Hz is no pitch): a frame
 * is voiced iff every knot np.interp reads for it — both bracketing ones, or the single one — has value > 0; voiced
 * frames get the interpolated value and vuv_out = 1, all others out = 0 and vuv_out = 0.  vuv_out (DEVICE, may be NULL)
 * is written in that mode only.  out must not alias tp. */
int wh_interp_contour(wh_ctx* ctx, void* stream, const wh_batch* b, const double* tp, const int64_t* h_knot_off,
                      const double* h_time, const double* h_value, int voiced_rule, double* out, double* vuv_out);
/* regrid_rows: a frame-major tensor in[src frames][k_bins] moved to another frame grid,
 * out[f'][k] = np.interp(tp_dst[f'], tp_src of u, in[frames of u][k]) for the utterance u of destination frame f' — `src`
 * and `dst` describe the same utterances (frame offsets of the two grids), no row of another utterance is ever read.
 * tp_src must be strictly increasing inside every utterance (the caller's check: it is device data); an utterance with
 * destination frames needs at least one source frame.  k_bins >= 1: spectrogram and aperiodicity rows, band rows, and
 * with k_bins = 1 per-frame scalars.  positive_rule != 0: the rule of wh_interp_contour per element — 0 unless every
 * source value read is > 0 (f0, vuv and gates: a gate stays 1 only where every source frame read has it).  The search
 * runs once per destination frame in a kernel of its own; the row kernel reads at most two source rows per output row.
 * out must not overlap in. */
int wh_regrid_rows(wh_ctx* ctx, void* stream, const wh_batch* src, const wh_batch* dst, const double* tp_src,
                   const double* tp_dst, const double* in, double* out, int k_bins, int positive_rule);

/* ---- Frame alignment of parallel utterances: batched dynamic time warping (no counterpart in the reference) ------------ */
/* Pair u aligns utterance u of `a` (N rows of xa) with utterance u of `b` (M rows of xb); rows are d doubles, row
 * strides lda / ldb >= d, 1 <= d <= 64.  The arithmetic is fixed (tests/_dtw_reference.py is the same
 * contract in NumPy, and the results agree bit for bit):
 *   c(i,j) = sqrt(s), s summed from 0.0 over k = 0..d-1 of (a[i][k]-b[j][k])*(a[i][k]-b[j][k]), unfused, sqrt correctly
 *     rounded;
 *   D(0,0) = c(0,0), otherwise D(i,j) = c(i,j) + best, best among the predecessors that exist in the order D(i-1,j-1),
 *     D(i-1,j), D(i,j-1), a later one replacing an earlier one only where it is strictly smaller; the one chosen is the
 *     cell's back-pointer;
 *   radius >= 1: cell (i,j) takes part iff |j*(N-1) - i*(M-1)| <= radius*max(N-1, M-1) (int64); the others hold +inf.
 *     radius <= 0: the whole rectangle;
 *   the path follows the back-pointers from (N-1,M-1) to (0,0) and is stored in forward order; on row 0 and on column
 *     0 the only existing predecessor is taken whatever the values, so a path is well formed for non-finite input too;
 *   map_b2a[j] = (i_lo + i_hi) / 2 over the path cells i_lo..i_hi that share j, map_a2b[i] likewise over those sharing i.
 * Outputs (DEVICE): path_a / path_b hold batch-global frame indices (local index + the side's frame offset); the path
 * of pair u occupies [h_path_off[u], h_path_off[u] + path_len[u]), and h_path_off (HOST) must leave each pair
 * N_u + M_u - 1 entries; path_len / total_cost [n_utt] (total_cost = D(N-1,M-1)); map_a2b [frames of a] and map_b2a
 * [frames of b] hold batch-global indices of the other side.  acc_out (may be NULL; a test hook for small shapes): D of
 * every pair, row-major N x M at h_acc_off[u] (HOST).  The back-pointers (two bits per cell, rows padded to 16 cells) and
 * the strip hand-off lines live in the context's scratch: the sum of 4 N_u ceil(M_u / 16) + 8 M_u bytes per call.  No atomics: a pair's result does not depend
 * on the batch it is in.  One wave per pair: 1024 pairs of 2001 x 2001 frames, d = 39, take 45.7 ms on one MI355X (27.6 % of the
 * FP64 vector issue rate), 23.7 ms inside radius 200; 64 pairs 40.8 ms.  Different utterance counts, an empty utterance on either side, d out of range or path offsets
 * that leave too little room fail before anything is launched. */
int wh_dtw(wh_ctx* ctx, void* stream, const wh_batch* a, const wh_batch* b, const double* xa, int64_t lda, const double* xb,
           int64_t ldb, int d, int64_t radius, const int64_t* h_path_off, int64_t* path_a, int64_t* path_b,
           int64_t* path_len, double* total_cost, int64_t* map_a2b, int64_t* map_b2a, double* acc_out,
           const int64_t* h_acc_off);

/* ---- Dynamic features and maximum-likelihood parameter generation (no counterpart in the reference) ------------------- */
/* What a statistical model of WORLD parameters is trained on and what turns its output back into a track.  Windows:
 * h_win[n_win][2*half+1] (HOST), 1 <= n_win <= 4, half L in {0, 1, 2}; window 0 must be the static window (centre tap
 * exactly 1.0, every other tap exactly 0.0: it gives W full column rank).  A tap that reaches outside its utterance is
 * dropped (np.correlate(.., 'same')); no row of another utterance is ever read.  The arithmetic is fixed (DESIGN section
 * 15; tests/_mlpg_reference.py is the same contract in NumPy, and the results agree bit for bit); every sum starts from
 * 0.0 and is unfused, every product is rounded on its own and grouped as written:
 *   features:  out[s][w*d + c] = sum over a = -L..L ascending with 0 <= s+a < T of win[w][a+L] * x[s+a][c];
 *   generation, per system (utterance u of T frames, column c), band half-width B = 2L:
 *     p_w[s] = 1.0 / var[s][w*d + c]  (one correctly rounded division);
 *     R[t][t+k] = sum over w ascending, then s ascending in max(0, t+k-L) .. min(T-1, t+L), of
 *                 (win[w][t-s+L] * p_w[s]) * win[w][t+k-s+L],   k = 0..B, t+k < T;
 *     r[t]      = sum in the same order over s in max(0, t-L) .. min(T-1, t+L) of (win[w][t-s+L] * p_w[s]) * mean[s][w*d + c];
 *     a sequential banded LDL^T without square roots, row t ascending with m = min(B, t); l[t][k] is the multiplier
 *     L[t][t-k], q[t] = 1.0 / d[t] the pivot's only division, and every subtraction runs from the farthest predecessor
 *     to the nearest:
 *       for k = m .. 1:  v_k = R[t-k][t];  for n = m .. k+1: v_k -= v_n * l[t-k][n-k];  l[t][k] = v_k * q[t-k];
 *       d[t] = R[t][t];  for k = m .. 1: d[t] -= v_k * l[t][k];      q[t] = 1.0 / d[t];
 *       z[t] = r[t];     for k = m .. 1: z[t] -= l[t][k] * z[t-k];   y[t] = z[t] * q[t]   (the same sweep);
 *     then from t = T-1 down:  c[t] = y[t];  for k = min(B, T-1-t) .. 1: c[t] -= l[t+k][k] * c[t+k].
 * A pivot that is not a positive finite number raises WH_FLAG_MLPG_PIVOT; the call still returns, every access stays in
 * range, and the other systems are untouched (a system's result never depends on the batch it is in).  An utterance
 * without frames produces nothing.  x / mean / var / out: DEVICE, frame-major, row strides >= the row width (d for x and
 * wh_mlpg's out, n_win*d for mean, var and wh_delta_features' out); ldv == 0: var is ONE row of n_win*d variances used for
 * every frame.  d >= 1.  pivots_out (may be NULL; a test hook): d[t] of every system, [total_frames][d].  wh_mlpg keeps the
 * multipliers in the context's scratch, 2L * 8 bytes per frame and column (y is kept in out), and out must not overlap
 * mean or var.  One lane per system, 64 consecutive
 * systems (u * d + c) per wave; the measured times are in DESIGN section 15.  Wrong arguments fail before anything is
 * launched. */
int wh_delta_features(wh_ctx* ctx, void* stream, const wh_batch* b, const double* x, int64_t ldx, int d, int n_win, int half,
                      const double* h_win, double* out, int64_t ldo);
int wh_mlpg(wh_ctx* ctx, void* stream, const wh_batch* b, const double* mean, int64_t ldm, const double* var, int64_t ldv,
            int d, int n_win, int half, const double* h_win, double* out, int64_t ldo, double* pivots_out);

/* ---- Joint-density Gaussian mixtures for voice conversion (no counterpart in the reference's library) ------------------ */
/* The frame-proportional parts of EM on joint vectors and of the conversion (Toda, Black and Tokuda 2007; DESIGN section
 * 16; tests/_gmm_reference.py is the same contract in NumPy).  Every matrix is row-major FP64 on the DEVICE; rows of x have
 * a stride ldx >= their width.  1 <= d <= 160, 1 <= M <= 64; a limit exceeded, a stride below the row width or a null
 * pointer where one is needed fails before anything is launched; n_rows == 0 is no error and launches nothing.  The three
 * products run on the FP64 matrix cores, so a sum's order and fusing are not part of the contract: results are held to
 * error bounds derived from the operands, and are exact where every partial sum is.  A row's result never depends on the
 * other rows of the call; non-finite input flows through as NaN or +-inf, and no index or trip count depends on a value.
 *   wh_gmm_estep:  mu [M][d], whiten [M][d][d] = W_m = L_m^-T (upper triangular; the lower triangle is not read above
 *     the 16 x 16 blocks of the diagonal and must hold zeros), logc [M] = log w_m - sum log diag L_m - (d/2) log 2 pi.
 *       z = (x_n - mu_m) W_m;  ll[n][m] = logc[m] - 0.5 sum_j z_j^2;
 *       mx = max_m ll;  s = sum over m ascending of exp(ll[n][m] - mx);  rowll[n] = mx + log s;
 *       gamma[n][m] = exp(ll[n][m] - mx) / s;  best[n] = the smallest m that attains mx (int32).
 *     exp and log are the device library's (<= 1 ulp).  ll (row stride ldl >= M), gamma (ldg >= M), rowll and best may
 *     each be NULL.
 *   wh_gmm_stats:  gamma [n_rows][M] with stride ldg, mu [M][d] the centre of each component;
 *       s0[m] = sum_n gamma;  s1[m][i] = sum_n gamma (x_i - mu_mi);  s2[m][i][j] = sum_n gamma (x_i - mu_mi)(x_j - mu_mj).
 *     Both triangles of s2 are written and agree bit for bit.  The rows are summed in consecutive runs of 4096 whose
 *     partial results ([run][m][d+1][d+1], wh_gmm_workspace_bytes(n_rows, d, M) bytes of the context's scratch) are
 *     added in ascending order: no atomics, the same input gives the same bits on every run.
 *   wh_gmm_convert:  x [n_rows][dx], mu_x [M][dx], a [M][dx][dy] = A_m = Sigma_xx^-1 Sigma_xy, mu_y [M][dy]; dx, dy >= 1,
 *     dx + dy <= 160.  Exactly one of best (int32 [n_rows]) and g ([n_rows][M], stride ldg) is given:
 *       best:  out[n] = mu_y[m] + (x_n - mu_x[m]) A_m  for m = best[n]  (a value outside [0, M) gives a row of zeros);
 *       g:     out[n] = sum over m ascending of g[n][m] * (mu_y[m] + (x_n - mu_x[m]) A_m)   (the MMSE conversion),
 *              evaluated as one accumulation of (g[n][m] (x_n - mu_x[m])) A_m over all m and k with sum_m g[n][m] mu_y[m]
 *              behind it.
 *     out has the row stride ldo >= dy and must not overlap an input.
 *   wh_gmm_workspace_bytes: host only; -1 for arguments outside the limits. */
int wh_gmm_estep(wh_ctx* ctx, void* stream, const double* x, int64_t n_rows, int64_t ldx, int d, int M, const double* mu,
                 const double* whiten, const double* logc, double* ll, int64_t ldl, double* gamma, int64_t ldg,
                 double* rowll, int32_t* best);
int wh_gmm_stats(wh_ctx* ctx, void* stream, const double* x, int64_t n_rows, int64_t ldx, int d, int M, const double* gamma,
                 int64_t ldg, const double* mu, double* s0, double* s1, double* s2);
int wh_gmm_convert(wh_ctx* ctx, void* stream, const double* x, int64_t n_rows, int64_t ldx, int dx, int dy, int M,
                   const double* mu_x, const double* a, const double* mu_y, const int32_t* best, const double* g,
                   int64_t ldg, double* out, int64_t ldo);
int64_t wh_gmm_workspace_bytes(int64_t n_rows, int d, int M);

/* ---- Line spectral frequencies: all-pole coding of the envelope at any rate (no counterpart in the reference's library) -- */
/* Per frame and independent; tests/_lsf_reference.py is the same contract in NumPy and the results agree
 * bit for bit.  Every sum is sequential and unfused, every product is rounded on its own and grouped as written, and no
 * kernel evaluates a transcendental: the kernels work on x = cos w and the only trigonometry is the HOST tables below.
 * The autocorrelation lags 0..p of a power-spectrum row are wh_feature_matmul with the table w_k cos(2 pi k m / N) / N.
 *   wh_lpc_levinson:  r [n_frames][ldr >= p+1] -> a [n_frames][lda >= p+1] (a[0] = 1), e [n_frames] (the prediction
 *     error), refl (may be NULL) [n_frames][ldk >= p] the reflection coefficients; 1 <= p <= 64.
 *       E = r[0];  for n = 1..p:  acc = r[n];  for i = 1..n-1 ascending: acc += a[i] * r[n-i];  k = -(acc / E);
 *       for i = 1..n/2: (a[i], a[n-i]) = (a[i] + k * a[n-i], a[n-i] + k * a[i]);  a[n] = k;  E = E * (1.0 - k * k).
 *     r[0] == 0 exactly: a = e0, E = 0, refl = 0, no flag.  r[0] negative or not finite, or an E after any order that
 *     is not positive and finite: that frame's outputs are NaN and WH_FLAG_LSF is raised; other frames are untouched.
 *   wh_lsf_from_lpc:  a [n_frames][lda >= p+1] -> x [n_frames][ldx >= p], the cosines of the line spectral frequencies
 *     in descending order (w ascending); p even, 2 <= p <= 64.  With m = p/2: g[0] = h[0] = a[0],
 *     g[i] = (a[i] + a[p+1-i]) - g[i-1], h[i] = (a[i] - a[p+1-i]) + h[i-1] (P and Q without their trivial roots); the
 *     series c[0] = g[m], c[k] = 2.0 * g[m-k] (the same with h) is evaluated by Clenshaw's recurrence
 *       b1 = b2 = 0;  for k = m..1: (b1, b2) = ((2.0 * x) * b1 - b2) + c[k], b1;   f = (x * b1 - b2) + c[0].
 *     h_grid[4097] (HOST) = cos(pi g / 4096).  Level G = 256, 512 .. 4096 looks at x_j = h_grid[j * 4096 / G], j = 0..G;
 *     a bracket is a j >= 1 with (f(x_j) < 0) != (f(x_(j-1)) < 0), the first m of each series are taken, and a level at
 *     which either series shows fewer than m gives way to the next; past 4096 the frame's row is NaN and WH_FLAG_LSF is
 *     raised.  A bracket is bisected at most 60 times: mid = 0.5 * (lo + hi), stop when mid equals an end, the half whose
 *     end shares the sign predicate of mid is dropped; the root is 0.5 * (lo + hi).  x[2i] is P's root i, x[2i+1] Q's.
 *     level_out (may be NULL; int32 [n_frames], a test hook): the level that found every root, 0 for a flagged frame.
 *   wh_lsf_envelope:  rows [n_frames][ldr >= p+1] = [E, x_1 .. x_p] -> out [n_frames][ldo >= k_bins], the power spectrum
 *     E / |A|^2 on k_bins = N/2 + 1 bins, in product form (the polynomial is never rebuilt); h_cos[k_bins] (HOST) =
 *     cos(pi k / (k_bins - 1)).  Per bin, c = h_cos[k]:  u = the product over i = 0, 2, .. of (2.0 * c - 2.0 * x[i]) from
 *     1.0, v the same over i = 1, 3, ..;  A2 = 0.25 * ((2.0 * (1.0 + c)) * (u * u) + (2.0 * (1.0 - c)) * (v * v));
 *     out = E / A2.  Rows are used as they are (world.lsf.ilsf_device repairs unsorted rows on request, in radians).
 * All matrices DEVICE, FP64.  n_frames == 0 is no error.  Wrong arguments fail before anything is launched. */
int wh_lpc_levinson(wh_ctx* ctx, void* stream, const double* r, int64_t n_frames, int64_t ldr, int p, double* a, int64_t lda,
                    double* e, double* refl, int64_t ldk);
int wh_lsf_from_lpc(wh_ctx* ctx, void* stream, const double* a, int64_t n_frames, int64_t lda, int p, const double* h_grid,
                    int n_grid, double* x, int64_t ldx, int32_t* level_out);
int wh_lsf_envelope(wh_ctx* ctx, void* stream, const double* rows, int64_t n_frames, int64_t ldr, int p, const double* h_cos,
                    int k_bins, double* out, int64_t ldo);

/* ---- A chain over line spectral frequencies: repair and scoring (no counterpart in the reference's library) ------------- */
/* Per frame / per pair and independent; tests/_lsf_chain_reference.py is the same contract in NumPy.
 *   wh_lsf_repair:  w [n_frames][ldw >= p] angles in radians -> out [n_frames][ldo >= p], decodable: inside [gap, hi]
 *     and at least gap apart; 2 <= p <= 64, gap > 0, hi >= gap (world.lsf passes min_gap and the double pi - min_gap).
 *     out == w (in place) is allowed; otherwise the two must not overlap.  In this order, max / min giving NaN when
 *     either operand is one (torch.maximum / minimum, not fmax / fmin), every + and - rounded once:
 *       1. w[i] = min(max(w[i], gap), hi) for every i;     2. w[i] = max(w[i], w[i-1] + gap), i = 1 .. p-1 ascending;
 *       3. w[p-1] = min(w[p-1], hi);                        4. w[i] = min(w[i], w[i+1] - gap), i = p-2 .. 0 descending.
 *     The result equals world.lsf.repair_rows bit for bit.  changed (may be NULL; int32 [n_frames]): the number of
 *     angles of the frame whose output bits differ from the input bits.  No flag is raised; a frame's result depends on
 *     its own row only (a NaN spreads inside its row as the four steps carry it).
 *   wh_lsf_distortion:  rows_a [n_rows_a][lda >= p+1], rows_b [n_rows_b][ldb >= p+1] in wh_lsf_envelope's form
 *     [., x_1 .. x_p] (cosines, descending; column 0 is not read); p even, 2 <= p <= 64.  Pair n compares row idx_a[n] of
 *     a with row idx_b[n] of b (DEVICE int64 [n_pairs]; either may be NULL: row n).  h_cos[k_bins] (HOST) as for
 *     wh_lsf_envelope.  Per bin, c = h_cos[k]: u, v and A2 of each side exactly as wh_lsf_envelope forms them;
 *     q = A2_a / A2_b (one division); t = log q, the device library's logarithm (<= 1 ulp).
 *       out[n][0] = sum over the k_bins bins of t;   out[n][1] = sum of t * t.
 *     The order of the two sums is not part of the contract; it is fixed (no atomics), so the same pair gives the same
 *     bits on every run, alone or among other pairs.  Two identical rows give (0.0, 0.0) exactly.  An index outside
 *     [0, n_rows) reads nothing and gives that pair (NaN, NaN); a non-finite row, or a root that coincides with a bin's
 *     cosine, flows through as inf / NaN in that pair only.  out: DEVICE [n_pairs][2].
 * All matrices DEVICE, FP64.  n_frames == 0 / n_pairs == 0 is no error.  Wrong arguments fail before anything is launched. */
int wh_lsf_repair(wh_ctx* ctx, void* stream, const double* w, int64_t n_frames, int64_t ldw, int p, double gap, double hi,
                  double* out, int64_t ldo, int32_t* changed);
int wh_lsf_distortion(wh_ctx* ctx, void* stream, const double* rows_a, int64_t n_rows_a, int64_t lda, const double* rows_b,
                      int64_t n_rows_b, int64_t ldb, int p, const int64_t* idx_a, const int64_t* idx_b, int64_t n_pairs,
                      const double* h_cos, int k_bins, double* out);

/* ---- A per-frame spectral gain applied to a waveform: vocoder-free conversion (no counterpart in the reference's library) -- */
/* ABI 121; tests/_specfilter_reference.py is the same contract in NumPy.  The recording is cut into
 * Hanning windows on an integer hop, every window's spectrum is multiplied by the minimum-phase spectrum of a log-gain
 * row, and the responses are overlap-added: the frame loop of world/synthesisRequiem.py:74-101 as a filter for recordings.
 * Per utterance u: ny = h_x_off[u+1] - h_x_off[u] samples, F = h_frame_off[u+1] - h_frame_off[u] gain rows (rows
 * h_frame_off[u] .. of num and den), H = h_hop[u] >= 1 with 2 H - 1 <= fft_size = N, K = N / 2 + 1.
 *   windows   W = ceil(ny / H) + 1 (an empty utterance: none), w = 0 .. W-1; window w starts at the 0-based sample
 *             s_w = w H - H (centre w H - 1: synthesisRequiem.py:84);  win[j] = 0.5 - 0.5 cospi(2 (j + 1) / (2 H)),
 *             j < 2 H - 1 (win[j] + win[j + H] = 1).
 *   row map   window w uses gain row h_map[h_map_off[u] + w] of the utterance (HOST int32; h_map_off[u+1] - h_map_off[u]
 *             must be W); an entry outside [0, F) is an argument error.
 *   segment   seg[j] = x[s_w + j] * win[j] where 0 <= s_w + j < ny, else 0, zero-padded to N.  Nothing is clipped.
 *   gain      h[k], k < K, the half log power ratio of row r = map[w]:
 *             kind 0 (spectrum; p_or_kbins = K, rows of K bins): h = (log|num[r][k]| - log|den[r][k]|) / 2;
 *               den == NULL: h = log|num[r][k]| / 2.
 *             kind 1 (lsf; p_or_kbins = p, even, 2 .. 64; rows [log E, x_1 .. x_p], x = cos w descending, as
 *               wh_lsf_envelope takes them but with the LOG of the gain in column 0): per bin, c = h_cos[k] (HOST [K],
 *               cos(pi k / (K - 1))), A2 of each side exactly as wh_lsf_distortion forms it;
 *               h = ((logE_n - logE_d) - log(A2_n / A2_d)) / 2;  den == NULL: h = (logE_n - log A2_n) / 2.
 *             G_w = the minimum-phase spectrum of h: cepstrum of the mirrored h, fold (bin 0 kept, upper half doubled,
 *             lower half zeroed), exp of the inverse transform (synthesisRequiem.py:112-118).
 *   response  r_w = irfft(rfft(seg) * G_w), N real taps, circular;  y[t] = the sum over the windows with
 *             0 <= t - s_w < N of r_w[t - s_w], 0 <= t < ny.  Taps outside the utterance are dropped.
 * Not part of the contract: the order of that sum and the fusing inside the transforms (results are compared at
 * tolerances, as for wh_synthesis_requiem).  Part of it: no atomics — the same bits from run to run, and for an
 * utterance alone as inside any batch; non-finite or non-positive gain entries flow through (a NaN in gain row r
 * reaches the samples [s_w, s_w + N) of the windows with map[w] == r and nothing else); no index or trip count
 * depends on a value.  num, den (ldn, ldd: doubles between rows), x, y: DEVICE, FP64; y in x's layout, y must not
 * overlap x.  h_cos may be NULL for kind 0.  n_utt == 0 is no error; wrong arguments fail before anything is launched. */
int wh_spectral_filter(wh_ctx* ctx, void* stream, int n_utt, const int64_t* h_x_off, const int64_t* h_frame_off,
                       const int64_t* h_map_off, const int32_t* h_map, const int64_t* h_hop, int kind, const double* num,
                       int64_t ldn, const double* den, int64_t ldd, int p_or_kbins, const double* h_cos, int fft_size,
                       const double* x, double* y);

/* ---- The same filter with mel-cepstral gain rows, in closed form (no counterpart in the reference's library) ------------- */
/* ABI 127; tests/_melcep_reference.py is the same contract in NumPy.  Windows, row map, segment,
 * response, overlap-add, limits and everything under "part of the contract" are wh_spectral_filter's; only the gain
 * differs.  Rows are mel-cepstra c[0 .. m], m = order, 1 <= m <= 64 (any parity; ldn, ldd >= m + 1), on the axis of a
 * first-order all-pass warp alpha, -1 < alpha < 1: beta(w) = w + 2 atan2(alpha sin w, 1 - alpha cos w), beta_k =
 * beta(pi k / (K - 1)).  They code a POWER spectrum as log P[k] = 2 sum_j c[j] cos(j beta_k) (the SPTK convention).
 *   gain      d[j] = num[r][j] - den[r][j], j <= m, of row r = map[w] (den == NULL: num[r][j]);
 *             G_w[k] = exp(sum_j d[j] cos(j beta_k)) * cis(-sum_j d[j] sin(j beta_k)), k < K: the transfer function
 *             exp(sum_j d[j] z~^-j), z~^-1 = (z^-1 - alpha) / (1 - alpha z^-1), on the unit circle.  It is minimum phase
 *             as it stands: no logarithm, no cepstral fold, and neither envelope is ever in memory.
 *   tables    h_cos_beta[k] = cos(beta_k), h_sin_beta[k] = sin(beta_k): HOST [K] each, the caller's (world.melcep.warp_tables);
 *             the library computes no trigonometric table of its own and never sees alpha.
 * Not part of the contract: how the two sums are evaluated (one Clenshaw recurrence per bin, b_j = d[j] + 2 cos(beta) b_{j+1}
 * - b_{j+2}; re = d[0] + cos(beta) b_1 - b_2, im = sin(beta) b_1, which may fuse); results are compared at tolerances.
 * A NaN in row r reaches the samples [s_w, s_w + N) of the windows with map[w] == r and nothing else.  NULL tables, an
 * order outside [1, 64] and a leading dimension below order + 1 fail before anything is launched, like every other wrong
 * argument.  wh_spectral_filter itself keeps refusing kind 2. */
int wh_melcep_filter(wh_ctx* ctx, void* stream, int n_utt, const int64_t* h_x_off, const int64_t* h_frame_off,
                     const int64_t* h_map_off, const int32_t* h_map, const int64_t* h_hop, const double* num, int64_t ldn,
                     const double* den, int64_t ldd, int order, const double* h_cos_beta, const double* h_sin_beta,
                     int fft_size, const double* x, double* y);

/* ---- Waveform-similarity overlap-add: the timing of a recording changed without analysis and synthesis (no counterpart) -- */
/* ABI 122; tests/_wsola_reference.py is the same contract in NumPy.  Stretching a recording by the f0
 * ratio with this and resampling it back by the inverse ratio (wh_resample_poly) moves its f0 and keeps its duration: the
 * f0 transformation that vocoder-free conversion (wh_spectral_filter) needs between speakers of different pitch.
 * Per call: an integer hop H = hop, 1 <= H <= 1024; a tolerance D = tol, 0 <= D <= 512; L = 2 H - 1; a HOST window table
 * h_win[0 .. L) (the binder passes 0.5 - 0.5 cos(pi (j + 1) / H), the spectral filter's window: win[j] + win[j + H] = 1;
 * the library computes no table of its own).  Per utterance u: x[0 .. n), n = h_x_off[u+1] - h_x_off[u]; the output
 * y[0 .. n_out), n_out = h_y_off[u+1] - h_y_off[u]; M = ceil(n_out / H) + 1 frames (none when n_out == 0) and the HOST
 * list pos[0 .. M) = h_pos[h_pos_off[u] ..], the nominal input start of every frame (h_pos_off[u+1] - h_pos_off[u] must
 * be M).  Any int64 is a legal position: a read of x outside [0, n) is 0.0 everywhere below, nothing is clipped.
 *   chain     delta_0 = 0;  c_m = pos[m] + delta_m.  For m >= 1 the template is t[j] = x[c_{m-1} + H + j], j < L — the
 *             natural continuation of the frame before — and candidate d in [-D, D] is g_d[j] = x[pos[m] + d + j].
 *   score     num = sum_j t[j] * g_d[j], den = sum_j g_d[j] * g_d[j]: each sum from +0.0, j ascending, every product and
 *             every sum rounded on its own (no fused multiply-add);  score = num / sqrt(den) when den > 0, else 0.0
 *             (divide and square root correctly rounded);  a NaN score counts as -inf.
 *   choice    delta_m = the d of the greatest score; among equal scores the smallest |d|, then the negative one (a total
 *             order: digital silence and an all-NaN frame give delta = 0).
 *   output    with o_m = m H - H:  y[t] = sum over the frames with 0 <= t - o_m < L, m ascending, of
 *             win[t - o_m] * x[c_m + t - o_m], from +0.0 and unfused, 0 <= t < n_out (at most two terms).
 * Part of the contract: no atomics — the same bits from run to run, and for an utterance alone as inside any batch; the
 * only value-dependent index is delta, confined to [-D, D]; every access is range-tested; a NaN or Inf in x reaches no other
 * utterance.  The shifts and y are compared bit for bit with the reference.  h_*: HOST; x, y: DEVICE FP64 (y must not
 * overlap x); delta: DEVICE int32 [h_pos_off[n_utt]], the shifts, may be NULL.  The frames of an utterance are one
 * sequential chain (one workgroup per utterance): a small batch of long utterances leaves most of the device idle.
 * n_utt == 0 is no error; wrong arguments (the limits, offsets that decrease, a position list of another length than M) fail
 * before anything is launched, with the reason in wh_last_error. */
int wh_wsola(wh_ctx* ctx, void* stream, int n_utt, const int64_t* h_x_off, const int64_t* h_y_off, const int64_t* h_pos_off,
             const int64_t* h_pos, int hop, int tol, const double* h_win, const double* x, double* y, int32_t* delta);

/* ---- Pitch-synchronous overlap-add: a new f0 contour and timing for a recording (no counterpart) --------------------- */
/* ABI 125; tests/_psola_reference.py is the same contract in NumPy.  Grains two periods wide are cut
 * around pitch marks of the recording and re-spaced at the target period: the grain spacing sets f0, the grain content —
 * and with it the spectral envelope — stays.  Unlike wh_wsola + wh_resample_poly the target may be a contour, and the
 * formants do not move with f0.
 * Per call: grid G, 1 .. 4096, the spacing in samples of the three tracks; unvoiced_hop U, 1 .. 2048, the mark spacing
 * in unvoiced stretches; tol, 0 .. 512; pmin, 2 .. 2048, the smallest voiced period; smin, 1 .. 2048, the smallest
 * synthesis step; norm, 0 or 1.  PMAX = 2048.  eff(p) = p when pmin <= p <= PMAX, else 0 (unvoiced).  At most 65535
 * utterances per call (stage C's launch has one grid row per utterance).
 * Per utterance u: x[0 .. n), n = h_x_off[u+1] - h_x_off[u]; y[0 .. n_out), n_out = h_y_off[u+1] - h_y_off[u]; each at
 * most 2^40 samples, each mark list at most 2^31 - 1 entries; a read of x outside [0, n) is 0.0.  Three DEVICE tracks:
 * per_a (int32, Ka = n / G + 1 entries at h_pa_off[u]: the analysis period at input sample k G), per_s (int32,
 * Ks = n_out / G + 1 entries at h_ps_off[u]: the target period at output sample k G) and src (int64, Ks entries at
 * h_ps_off[u]: the input sample that output sample k G corresponds to, clamped to +- 2^62 before use).  The offsets'
 * differences must be Ka and Ks.  The tracks are data no host check sees: no value in them takes an access out of range
 * or a loop beyond its capacity.
 *   stage A   analysis marks, a sequential chain.  n == 0: none.  a_0 = 0.  At mark i: P_i = eff(per_a[min(Ka - 1, a_i / G)]).
 *             a_i >= n: the last mark, Ma = i + 1 (the mark at or beyond the end belongs to the list).  P_i == 0:
 *             a_{i+1} = a_i + U.  Otherwise h = P_i / 2, D_i = min(tol, P_i / 4), the template is t[j] = x[a_i - h + j],
 *             j < P_i, candidate d in [-D_i, D_i] is g_d[j] = x[a_i + P_i + d - h + j], and score and choice are wh_wsola's:
 *             num = sum t[j] g_d[j], den = sum g_d[j] g_d[j], from +0.0, j ascending, unfused; num / sqrt(den) when den > 0
 *             else 0.0; NaN counts as -inf; the greatest score, then the smallest |d|, then the negative one.
 *             a_{i+1} = a_i + P_i + d*.  Every step is at least m = min(U, pmin - min(tol, pmin / 4)), so
 *             Ma <= ceil(n / m) + 1: h_mark_off[u+1] - h_mark_off[u] must be at least that.
 *   stage B   synthesis marks, a sequential integer chain.  None when n_out == 0 or Ma == 0 (y is then +0.0).  s_0 = 0.
 *             At mark j: k = min(Ks - 1, s_j / G); c = src[k] + (s_j - k G); sel_j = the i that minimises |a_i - c|, the
 *             lower i on a tie (src need not be monotone); flip_j = 1 exactly when j >= 1, P_sel_j == 0,
 *             sel_j == sel_{j-1} and flip_{j-1} == 0 (a repeated unvoiced grain is read backwards).  s_j >= n_out: the
 *             last mark, Ms = j + 1.  Otherwise with Q = eff(per_s[k]): if Q > 0 and P_sel > 0, sp = a_{sel+1} - a_sel
 *             (P_sel at the last mark) and step = max(smin, (sp Q + P_sel / 2) / P_sel) in integers; else step = U.
 *             s_{j+1} = s_j + step.  h_smark_off[u+1] - h_smark_off[u] must be at least ceil(n_out / min(U, smin)) + 1.
 *   stage C   overlap-add, a gather.  Grain j has i = sel_j, fb = P_i if P_i > 0 else U, Lw = a_i - a_{i-1} (fb when
 *             i == 0), Rw = a_{i+1} - a_i (fb when i is the last mark).  With tau = t - s_j the grain contributes to y[t]
 *             iff -Lw < tau < Rw: u = |tau| / (tau < 0 ? Lw : Rw), one IEEE divide of two exact doubles;
 *             w = 1 - (u u) (3 - 2 u), every operation rounded on its own (within 0.01 of a Hanning half; complementary
 *             halves sum to 1; no transcendental); v = x[a_i + (flip_j ? -tau : tau)]; num += w v and W += w, j ascending,
 *             from +0.0, unfused.  y[t] = num / max(W, 1.0) when norm, else num; no grain gives +0.0.
 * Outputs besides y, all DEVICE and each may be NULL (the context's scratch then holds it): marks (int64) and mark_period
 * (int32, P_i) at h_mark_off[u]; n_marks (int32 [n_utt]); smarks (int64), sel (int32) and flip (uint8) at h_smark_off[u];
 * n_smarks (int32 [n_utt]).  Entries beyond the counts are not written.
 * Part of the contract: no atomics — the same bits from run to run, and for an utterance alone as inside any batch; every
 * access is range-tested; a NaN or Inf in x reaches only the outputs of the grains that read it and, through the scores,
 * the later marks of the same utterance — no other utterance.  h_*: HOST; y must not overlap x.  Stages A and B are one
 * sequential chain per utterance (one workgroup, one wave): a small batch of long utterances leaves most of the device
 * idle; stage C is chip-wide.  n_utt == 0 is no error; wrong arguments (the limits, offsets that decrease, a track of
 * another length, a capacity too small) fail before anything is launched, with the reason in wh_last_error. */
int wh_psola(wh_ctx* ctx, void* stream, int n_utt, const int64_t* h_x_off, const int64_t* h_y_off, const int64_t* h_pa_off,
             const int64_t* h_ps_off, const int64_t* h_mark_off, const int64_t* h_smark_off, int grid, int unvoiced_hop,
             int tol, int pmin, int smin, int norm, const double* x, const int32_t* per_a, const int32_t* per_s,
             const int64_t* src, double* y, int64_t* marks, int32_t* mark_period, int32_t* n_marks, int64_t* smarks,
             int32_t* sel, uint8_t* flip, int32_t* n_smarks);

/* ---- Exemplar-based conversion: k-nearest-neighbour search and frame selection by Viterbi (no counterpart) ------------ */
/* ABI 124; tests/_exemplar_reference.py is the same contract in NumPy.  The target speaker's aligned
 * frames are kept as a database; every source frame takes the K entries whose source side is nearest (wh_knn), and a
 * Viterbi pass picks one per frame, trading closeness against the continuity of the chosen target frames
 * (wh_frame_select): every converted envelope is a frame the target speaker produced, nothing is averaged.
 *
 * wh_knn: q [n_q] rows of d columns with row stride ldq, db [n_db] rows with row stride lddb (DEVICE FP64; the strides
 * in elements, >= d: column slices are fine); 1 <= d <= 160, 1 <= K <= 32, n_db <= 2^31 - 1.
 *   distance  s(n, r) = sum over c = 0 .. d-1 ascending, from +0.0, of (q[n][c] - db[r][c]) * (q[n][c] - db[r][c]): every
 *             difference, product and sum rounded on its own (wh_dtw's local cost without the square root).
 *   key       s, or +inf where s is NaN.
 *   result    the candidates of query n are all rows r, less those with excl_lo[n] <= r < excl_hi[n] when the two DEVICE
 *             int32 arrays [n_q] are given (both or neither).  idx[n][0 .. K) (DEVICE int32, row stride K) are the K
 *             candidates that are smallest under the total order (key ascending, then r ascending), in that order;
 *             dist[n][k] (DEVICE FP64) is the key.  Slots beyond the number of candidates hold idx = -1, dist = +inf.
 *   splits    0: the library's choice; n >= 1 (at most 65535): the database is cut into n consecutive ranges of
 *             ceil(n_db / n) rows, every range keeps a list of its own and a second kernel merges the lists under the same
 *             order.  Because the order is total, neither the cut nor the tiling shows in the result: every value of
 *             splits gives the same bytes.
 * Part of the contract: no atomics; a query's result does not depend on the other queries of the call; no address and no
 * trip count depends on a feature value (the lists are updated by K compare-selects).  n_q == 0 or n_db == 0 is no error
 * (n_db == 0: every slot is empty).  Wrong arguments — a limit exceeded, a stride below d, a null pointer where one is
 * needed, one exclusion array without the other, splits < 0 — fail before anything is launched, with the reason in
 * wh_last_error. */
int wh_knn(wh_ctx* ctx, void* stream, const double* q, int64_t n_q, int64_t ldq, const double* db, int64_t n_db, int64_t lddb,
           int d, int K, const int32_t* excl_lo, const int32_t* excl_hi, int splits, int32_t* idx, double* dist);

/* wh_frame_select: per utterance of b (its frame offsets; F frames) one slot of every frame's K candidates.  idx, tc
 * [total_frames][K] are wh_knn's two outputs (DEVICE); y [n_db] rows of dy columns with row stride ldy >= dy (DEVICE FP64,
 * 1 <= dy <= 64); succ [n_db] (DEVICE int32) is the database row that follows each row in the target recording; weight is
 * finite and >= 0.
 *   validity  a slot with idx < 0 or idx >= n_db is invalid: its rows are never read and its accumulated cost is +inf.  As
 *             a predecessor, slot j of frame t-1 is also invalid where succ[idx(t-1, j)] lies outside [0, n_db).  The
 *             caller guarantees that slot 0 of every frame is valid.
 *   chain     A(0, k) = tc(0, k).  For t >= 1 and valid k: cc(j, k) = sum over c ascending, from +0.0, of the squared
 *             difference of y[idx(t, k)][c] and y[succ[idx(t-1, j)]][c], unfused;  v(j) = A(t-1, j) + weight * cc(j, k), one
 *             product and one sum, each rounded, and +inf for an invalid j;  best = v(0), and for j = 1 .. K-1 ascending
 *             v(j) replaces it only where strictly smaller (a NaN never replaces);  A(t, k) = tc(t, k) + best, the chosen j
 *             is the back-pointer (one byte per frame and slot in the context's scratch).
 *   end       the smallest k whose A(F-1, k) is strictly smallest (the same scan over k).
 *   outputs   sel[f] (DEVICE int32 [total_frames]) = idx of the chosen slot; slot[f] the slot, may be NULL;
 *             total[u] (DEVICE FP64 [n_utt]) = A(F-1, k*), 0.0 for an empty utterance; acc_out, may be NULL: A as
 *             [total_frames][K], a test hook like wh_dtw's.
 * Non-finite rows give unspecified values and a well-formed selection (ties and NaNs fall to slot 0).  An utterance's
 * result does not depend on the batch it is in; no atomics; the results repeat bit for bit.  One workgroup per utterance:
 * the frames are one sequential chain.  Wrong arguments fail before anything is launched. */
int wh_frame_select(wh_ctx* ctx, void* stream, const wh_batch* b, const int32_t* idx, const double* tc, int K, const double* y,
                    int64_t n_db, int64_t ldy, int dy, const int32_t* succ, double weight, int32_t* sel, int32_t* slot,
                    double* total, double* acc_out);

/* ---- 16-bit PCM at the batch boundary (the reference's WAV usage: example/prosody.py:12-13,57) ---------------------- */
/* x[i] = pcm[i] / (2^15 - 1); pcm[i] = int16(trunc(y[i] * 2^15)) (low 16 bits, like NumPy's astype on the reference's
 * platform).  DEVICE pointers: the 2-byte samples cross PCIe instead of the 8-byte ones. */
int wh_pcm16_to_f64(wh_ctx* ctx, void* stream, const int16_t* pcm, int64_t n, double* x);
int wh_f64_to_pcm16(wh_ctx* ctx, void* stream, const double* y, int64_t n, int16_t* pcm);

/* ---- Polyphase resampling in front of the analysis: replaces scipy.signal.resample_poly  (example/prosody.py:16-19) ---- */
/* y = resample_poly(x, up, down) per utterance of a ragged batch, bit for bit with scipy's defaults (window=('kaiser',
 * 5.0), padtype='constant', cval=None): upfirdn's loop — output j sums x[k] * h_trans_flip[(j*down) % up][.] over
 * k = (j*down)/up - P + 1 .. (j*down)/up in ascending order, each product rounded on its own, taps of k outside the
 * signal skipped — and output i of utterance u is upfirdn's j = i + h_pre_remove[u].
 *   h_in_off[n_utt+1], h_out_off[n_utt+1] (HOST, int64, monotone): sample offsets into x and y; n_out of utterance u
 *     must be ceil(n_in * up / down) (an empty utterance gives an empty output);
 *   h_up[u], h_down[u] (HOST): positive, at most 4096 (pass them reduced by their gcd, as resample_poly does);
 *   h_filters[n_filters] (HOST): the padded FIRs as resample_poly builds them (firwin(2*half+1, 1/max(up, down),
 *     window) * up behind n_pre_pad zeros and ahead of n_post_pad zeros); utterance u uses h_filters[h_filt_off[u] ..
 *     + h_filt_len[u]), and h_pre_remove[u] = (half + n_pre_pad) / down.  P = ceil(h_filt_len / up).  The phase tables
 *     are built here and cached in the context's bounded table cache by content.
 * x, y: DEVICE.  Asynchronous (the first call with a new filter uploads its table synchronously). */
int wh_resample_poly(wh_ctx* ctx, void* stream, int n_utt, const int64_t* h_in_off, const int64_t* h_out_off,
                     const int32_t* h_up, const int32_t* h_down, const int64_t* h_filt_off, const int64_t* h_filt_len,
                     const int64_t* h_pre_remove, const double* h_filters, int64_t n_filters, const double* x, double* y);

#ifdef __cplusplus
}
#endif
#endif /* WORLD_HIP_H */
