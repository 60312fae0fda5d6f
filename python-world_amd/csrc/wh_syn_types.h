// What the synthesis units share (wh_timebase.hip, wh_synthesis.hip, wh_requiem.hip): the per-utterance and per-pulse
// records, the frame-time interpolation, the workspace layout of the time base and the host helpers that cross units.
// Include after wh_host.h and wh_device.h.
#pragma once

namespace wh {

struct SynUtt {
  int64_t f_off, nf;      // frames
  int64_t y_off, ny;      // output samples
  int64_t p_off, pcap;    // pulse slots
  int64_t noise_off, noise_len;  // host-supplied noise stream (if any)
  double t0, dt;          // time axis t_i = t0 + i*dt  (NumPy arange semantics, host-computed)
};

// searchsorted-left, hi clipped to [1, nf-1]: the segment SciPy's interp1d(linear, extrapolate) evaluates t on.
// The frame times are almost always an even grid (also after scale_duration), so the answer is first guessed from the
// grid's mean step and checked against its definition (tp[lo-1] < t <= tp[lo]): two rounds of independent loads
// instead of log2(nf) dependent ones; any other time axis falls through to the bisection.  Same result either way.
__device__ __forceinline__ int64_t lerp_segment(const double* __restrict__ tp, int64_t nf, double t) {
  int64_t lo = 0, hi = nf;
  if (nf >= 2) {
    const double first = tp[0], last = tp[nf - 1];
    const double g = ceil((t - first) * (double)(nf - 1) / (last - first));
    if (g >= 1.0 && g <= (double)(nf - 1)) {
      const int64_t gi = (int64_t)g;
      const double a = tp[gi - 1], b = tp[gi], c = gi + 1 < nf ? tp[gi + 1] : b;
      if (a < t && !(b < t)) return gi;                                    // already inside [1, nf-1]
      if (b < t && !(c < t) && gi + 1 <= nf - 1) return gi + 1;
      if (gi >= 2 && !(a < t) && tp[gi - 2] < t) return gi - 1;
    }
  }
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (tp[mid] < t) lo = mid + 1; else hi = mid;
  }
  return lo < 1 ? 1 : (lo > nf - 1 ? nf - 1 : lo);
}
// slope*(t-x_lo)+y_lo on that segment
__device__ __forceinline__ double lerp_on(const double* __restrict__ tp, const double* __restrict__ v, int64_t ih, double t) {
  const int64_t il = ih - 1;
  const double slope = (v[ih] - v[il]) / (tp[ih] - tp[il]);
  return slope * (t - tp[il]) + v[il];
}

// Exclusive prefix of c over a 256-thread workgroup and the workgroup total (wsum: 4 ints of LDS).
__device__ __forceinline__ int block_excl_scan_256(int c, int* wsum, int* total) {
  int incl = c;
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int uu = __shfl_up(incl, o, 64);
    if (lane >= o) incl += uu;
  }
  __syncthreads();
  if (lane == 63) wsum[threadIdx.x >> 6] = incl;
  __syncthreads();
  int excl = incl - c, tot = 0;
  for (int w = 0; w < 4; ++w) {
    if (w < (int)(threadIdx.x >> 6)) excl += wsum[w];
    tot += wsum[w];
  }
  *total = tot;
  return excl;
}

// Everything response_kernel has to know about a pulse before it can touch the spectra, packed by the time base so that
// a workgroup gets it with ONE 64-byte scalar load — and gets the NEXT pulse's under the current pulse's row fetch —
// where it used to walk p_utt -> meta / p_base / p_count -> p_idx, p_shift, p_frames, p_weight, p_noff -> vuv_s: four
// dependent round trips in front of every pulse.
struct alignas(64) PulseRec {
  int64_t pidx;        // 1-based output index of the pulse (pulse_locations_index)
  int64_t rows;        // absolute spectrogram rows: (f_off + earlier frame) | (f_off + later frame) << 32
  double weight;       // of the later frame; -1: both frames are the same one
  double shift;        // pulse_locations_time_shift
  int64_t noff;        // offset of the pulse's noise run in the utterance's stream
  int32_t u;           // utterance
  int32_t noise_size;  // next pulse's index - this one's (0 for the last)
  int32_t vuv;         // interpolated vuv at the pulse (synthesis.py:69 reads it at pidx - 1)
  int32_t pad_[3];
};
static_assert(sizeof(PulseRec) == 64, "one 64-byte scalar load");

// First pulse of an utterance at or behind 1-based index `lo` (its pulse indices are ascending): a 64-ary search by the
// whole wave — probes at 64 evenly spaced pulses, a ballot, the same again inside the bracket — two rounds of loads for
// the few thousand pulses of an utterance where a bisection takes twelve dependent ones.  Wave-uniform.
__device__ __forceinline__ int first_pulse_at(const int64_t* __restrict__ pi, int count, int64_t lo) {
  const int lane = threadIdx.x & 63;
  int base = 0, n = count;  // the answer is in [base, base + n]
  while (n > 0) {
    const int stride = (n + 63) / 64;
    const int idx = base + lane * stride;
    const bool below = idx < base + n && pi[idx] < lo;
    const int c = __popcll(__ballot(below));  // the probes are ascending: the first c of them are below
    if (stride == 1) {
      base += c;
      break;
    }
    if (c == 0) break;  // pi[base] >= lo
    const int nb_ = base + (c - 1) * stride + 1;
    const int left = base + n - nb_;
    n = stride - 1 < left ? stride - 1 : left;
    base = nb_;
  }
  return base;
}

// ---- host side ------------------------------------------------------------------------------------------------------
// (wh::dispatch_fft_size, the switch over the kernels' transform lengths: wh_host.h)
// The front of every synthesis workspace, taken from `c` (the caller's own regions follow from the same carve): phase
// increments / cumulative phase, per-sample voicing, then per pulse slot the time, 1-based index, fractional shift and
// noise offset, the pulse counts and the pulse stage's scratch — crossing masks (one byte per 4 samples) and per-tile
// counts (wh_timebase.hip: launch_pulses).
struct TimeBaseLayout {
  Region<double> phase, pt, ps;
  Region<int64_t> pi, pn;
  Region<int32_t> pc, tile_cnt;
  Region<uint8_t> vuv, masks;
  TimeBaseLayout(Carve& c, int B, int64_t ny_tot, int64_t pulse_cap, int64_t max_ny);
};

// meta[u] of every utterance of the batch (noise == nullptr: no host noise stream) and the longest output.
int fill_syn_meta(const char* who, const wh_batch* b, const int64_t* h_y_off, const double* h_t0, const double* h_dt,
                  int64_t pulse_cap, const double* noise, const int64_t* h_noise_off, std::vector<SynUtt>& meta,
                  int64_t* max_ny);
// In-place exact cumulative sum of n_seg segments of d_data (h_off: n_seg + 1 HOST offsets), bit-identical to np.cumsum.
int exact_cumsum_segments(wh_ctx* ctx, hipStream_t st, double* d_data, const int64_t* h_off, int n_seg);
// prep_kernel, the exact phase scan and the pulse kernels into the buffers of `lay` in the workspace `ws`.
int launch_pulses(wh_ctx* ctx, hipStream_t st, int B, int64_t max_ny, const SynUtt* d_meta, const double* tp,
                  const double* f0, const double* vuv, double fs, double f0_low_limit, const int64_t* h_y_off, void* ws,
                  const TimeBaseLayout& lay);

}  // namespace wh
