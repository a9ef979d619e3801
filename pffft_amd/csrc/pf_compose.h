// The one host path of the entries that are COMPOSED on top of pf::Setup (frames_tu.hip, psd_tu.hip, csd_tu.hip, pfb_tu.hip, dct_tu.hip,
// mdct_tu.hip; through bluestein_host.h any_tu.hip, zoom_tu.hip, analytic_tu.hip, xcorr_tu.hip; through fft2d_host.h fft2_tu.hip,
// rfft2_tu.hip): how much scratch one launch sequence may hold, how a batch walks through it, how a fused launch is cut into slices, the
// overlap test of two address ranges, the selector rule of a fused / composed pair, the launch of an element-wise kernel, the frame-matrix
// routes of analysis and synthesis, the run walk of the averages, the lookup of the register-tiled configuration a fused kernel must share
// with transform_batch, and the handle that owns inner setups with their device test and typed public entries.  Every decision is written
// here once; each unit keeps its validation texts, its measured defaults and the arguments of its kernels.  Every function is internal to
// its includer.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/pffft_hip.h"
#include "pf_launch.h"
#include "fft_frames.h"

namespace pf {

// ------------------------------------------------------------------------------------------------ planners, on plain integers
// The scratch of one composed launch sequence (frame matrix, partial buffer, scratch image) holds at most this many bytes
// (include/pffft_hip.h): longer batches go through it in chunks on the stream.
constexpr size_t SCRATCH_CAP_BYTES = (size_t)256 << 20;
// The fused kernels count rows in 32 bits: longer batches go out in slices of this many rows on the same stream.
constexpr size_t ROW_SLICE = (size_t)3 << 30;

// rows that fit under the cap: one where a single row is longer
constexpr size_t cap_rows(size_t row_bytes, size_t cap = SCRATCH_CAP_BYTES) { return cap / row_bytes > 1 ? cap / row_bytes : 1; }
// rows per chunk of a batch that goes through the scratch
constexpr size_t chunk_rows(size_t batch, size_t row_bytes, size_t cap = SCRATCH_CAP_BYTES) {
    return batch < 1 ? 1 : batch < cap_rows(row_bytes, cap) ? batch : cap_rows(row_bytes, cap);
}
static_assert(chunk_rows(100, 16384) == 100, "a batch under the cap: one chunk");
static_assert(chunk_rows(20000, 16384) == 16384, "real float N = 4096: 16384 rows per chunk");
static_assert(chunk_rows(5, SCRATCH_CAP_BYTES + 1) == 1, "a row longer than the cap goes alone");
static_assert(chunk_rows(5, SCRATCH_CAP_BYTES / 2) == 2 && chunk_rows(5, SCRATCH_CAP_BYTES / 2 + 1) == 1, "both sides of an exact division");

// body(first row, rows) -> 0 or an error, for consecutive slices of at most ROW_SLICE rows
template <class Body>
constexpr int for_slices(size_t rows, Body&& body) {
    for (size_t b0 = 0; b0 < rows; b0 += ROW_SLICE)
        if (int rc = body(b0, rows - b0 < ROW_SLICE ? rows - b0 : ROW_SLICE)) return rc;
    return 0;
}
struct SliceWalk { size_t count, last; };
constexpr SliceWalk slice_walk(size_t rows) {
    SliceWalk w{0, 0};
    for_slices(rows, [&](size_t, size_t nb) { ++w.count; w.last = nb; return 0; });
    return w;
}
static_assert(slice_walk(ROW_SLICE).count == 1 && slice_walk(ROW_SLICE).last == ROW_SLICE, "3 x 2^30 rows: one slice");
static_assert(slice_walk(ROW_SLICE + 1).count == 2 && slice_walk(ROW_SLICE + 1).last == 1, "one row more: a second slice of that row");

// Synthesis beyond the cap goes signal by signal in runs of frames.  A run owns the samples from its first frame's start to the next
// run's first frame's start (the last run: to the end) and re-transforms the `reach` earlier frames that reach into them, so the matrix
// holds run + reach rows.  min_run is 0 for the frame entry: reach = ceil(N / hop) - 1 is small against any cap, and a run of one frame is
// correct.  The filter bank passes min_run = reach = ceil(taps N / hop) - 1, which grows with the taps: a run is then at least `reach` frames
// long, so that the re-transformed frames never outnumber the new ones, and where reach + 1 rows do not fit under the cap the matrix is
// as large as that takes (at most 2 reach rows).
constexpr size_t synth_reach(size_t span, size_t hop) { return (span + hop - 1) / hop - 1; }
struct RunPlan { size_t run, buffer_rows; };
constexpr RunPlan synth_plan(size_t nframes, size_t cap_rows_, size_t reach, size_t min_run) {
    size_t run = cap_rows_ > reach ? cap_rows_ - reach : 1;
    if (run < min_run) run = min_run;
    if (run < 1) run = 1;
    return {run, nframes < run + reach ? nframes : run + reach};
}
static_assert(cap_rows(4096 * 4) == 16384 && synth_reach(4096, 1024) == 3 && synth_reach(4 * 4096, 1024) == 15, "real float N = 4096, hop 1024");
static_assert(synth_plan(20000, 16384, 3, 0).run == 16381 && synth_plan(20000, 16384, 3, 0).buffer_rows == 16384, "... 20 000 frames");
static_assert(synth_plan(20000, 16384, 15, 15).run == 16369 && synth_plan(20000, 16384, 15, 15).buffer_rows == 16384, "... and taps 4");
static_assert(synth_plan(100, 2, 5, 0).run == 1 && synth_plan(100, 2, 5, 0).buffer_rows == 6, "cap <= reach, frames: one new frame per run");
static_assert(synth_plan(100, 2, 5, 5).run == 5 && synth_plan(100, 2, 5, 5).buffer_rows == 10, "cap <= reach, filter bank: 2 reach rows");

// The Welch averages (psd, csd) sum runs of AVG_RUN frames; a group of `navg` frames is rpg runs.  An average of one run is scaled and stored
// by the run itself.  Longer ones go through the partial buffer in whole groups: `vstep` of the V output rows per pass (a fused kernel counts
// the runs of a launch in 32 bits), then the reduction of those rows.  Composed, the frames of `crun` whole runs (of up to `lfull` frames) go
// through the frame matrix per chunk; frame_bytes: one frame row times the frame sets (csd: x and y, the cap holds for both together).
constexpr size_t AVG_RUN = PFFFT_HIP_PSD_RUN;   // (pf::PSD_RUN of fft_psd.h: psd_tu.hip and csd_tu.hip assert it)
struct AvgPlan { size_t V, navg; bool fused; size_t rpg, vstep, lfull, crun, part_rows, set_rows; };
constexpr AvgPlan avg_plan(size_t V, size_t navg, size_t part_row_bytes, size_t frame_bytes, bool fused) {
    AvgPlan p{V, navg, fused, (navg + AVG_RUN - 1) / AVG_RUN, V, std::min(navg, AVG_RUN), 0, 0, 0};
    if (p.rpg > 1) p.vstep = cap_rows(p.rpg * part_row_bytes);
    if (fused) p.vstep = std::min(p.vstep, std::max<size_t>(1, ROW_SLICE / p.rpg));
    p.vstep = std::min(p.vstep, V);
    p.crun = std::max<size_t>(1, cap_rows(frame_bytes) / p.lfull);
    p.part_rows = p.vstep * p.rpg;                                                   // rows of the partial buffer (taken where rpg > 1)
    p.set_rows = std::min(V * navg, std::min(p.crun, p.vstep * p.rpg) * p.lfull);    // rows of one set of the frame matrix (composed)
    return p;
}
// first frame of run r, in the numbering v = i nframes + f
constexpr size_t first_frame(size_t r, size_t navg, size_t rpg) { return (r / rpg) * navg + (r % rpg) * AVG_RUN; }
constexpr bool avg_is(const AvgPlan& p, size_t rpg, size_t vstep, size_t lfull, size_t crun, size_t part_rows, size_t set_rows) {
    return p.rpg == rpg && p.vstep == vstep && p.lfull == lfull && p.crun == crun && p.part_rows == part_rows && p.set_rows == set_rows;
}
// real float N = 4096: partial rows of P = 2049 (psd) or 2P (csd cross) scalars, frame rows of 4096 scalars in one set (psd) or two (csd)
static_assert(avg_is(avg_plan(7, 16, 8196, 16384, false), 1, 7, 16, 1024, 7, 112), "an average of one run; V smaller than vstep");
static_assert(avg_is(avg_plan(10, 32, 8196, 16384, false), 1, 10, 32, 512, 10, 320), "navg = 32: still one run");
static_assert(avg_is(avg_plan(10, 33, 8196, 16384, false), 2, 10, 32, 512, 20, 330), "navg = 33: two runs, the partial buffer");
static_assert(avg_is(avg_plan(10000, 100, 8196, 16384, false), 4, 8188, 32, 512, 32752, 16384), "psd, navg = 100: 8188 groups per pass");
static_assert(avg_is(avg_plan(10000, 100, 16392, 32768, false), 4, 4094, 32, 256, 16376, 8192), "csd cross, navg = 100: two sets");
static_assert(avg_is(avg_plan(100, 100, 16392, 32768, false), 4, 100, 32, 256, 400, 8192), "... 10 000 frames: 8192 rows per half");
static_assert(avg_plan(16377, 33, 8196, 16384, false).vstep == 16376 && avg_plan(8189, 33, 16392, 32768, false).vstep == 8188, "one group more: a second pass");
static_assert(avg_plan(5, 64, (size_t)1 << 26, 16384, false).vstep == 2 && avg_plan(5, 64, ((size_t)1 << 26) + 1, 16384, false).vstep == 1 &&
              avg_plan(5, 1, 8196, (size_t)1 << 27, false).crun == 2 && avg_plan(5, 1, 8196, ((size_t)1 << 27) + 1, false).crun == 1,
              "both sides of an exact division of the cap: by the partial rows of a group, by the frame rows");
static_assert(avg_is(avg_plan(5, 100, 8196, SCRATCH_CAP_BYTES + 1, false), 4, 5, 32, 1, 20, 32), "a row longer than the cap: one run per chunk");
static_assert(avg_plan(ROW_SLICE + 1, 16, 8196, 16384, true).vstep == ROW_SLICE && avg_plan(ROW_SLICE + 1, 16, 8196, 16384, false).vstep == ROW_SLICE + 1 &&
              avg_plan(10, (size_t)1 << 37, 4, 16384, true).vstep == 1, "a fused launch holds at most ROW_SLICE runs, and at least one group");
static_assert(first_frame(3, 100, 4) == 96 && first_frame(4, 100, 4) == 100 && first_frame(7, 100, 4) == 196 && first_frame(5, 16, 1) == 80, "a group of 100: runs of 32, 32, 32, 4");

// ------------------------------------------------------------------------------------------------ guards
// Do the byte ranges [a, a + alen) and [b, b + blen) share a byte?  Each entry keeps its own guard (in != out, batch != 0) and text.
constexpr bool ranges_overlap(uintptr_t a, size_t alen, uintptr_t b, size_t blen) { return a < b + blen && b < a + alen; }
static_assert(!ranges_overlap(0, 64, 64, 64) && !ranges_overlap(64, 64, 0, 64), "touching ranges, either one first");
static_assert(ranges_overlap(0, 65, 64, 64) && ranges_overlap(64, 64, 0, 65), "one byte of overlap, either one first");
static_assert(ranges_overlap(0, 256, 64, 16) && ranges_overlap(64, 16, 0, 256), "one range inside the other");
static_assert(!ranges_overlap(0, 16, 16, 256) && ranges_overlap(0, 17, 16, 256) && !ranges_overlap(272, 16, 16, 256) && ranges_overlap(271, 16, 16, 256),
              "different lengths: each side ends by its own");

// The selector rule of a fused / composed pair: composed where the kernel cannot run or the composed selector asks; else fused where the
// fused selector asks or the unit's measured default (its *_fused_default table) says so.
inline bool fused_selected(const AbSel& sel, AbValue composed, AbValue fused, bool fusable, bool by_default) {
    if (!fusable || sel.is(composed)) return false;
    return sel.is(fused) || by_default;
}

// ------------------------------------------------------------------------------------------------ shared launches
inline int bad_in(const char* prefix, const char* what, hipError_t e = hipErrorInvalidValue) {
    return bad((std::string(prefix) + what).c_str(), e);
}

// grid of a grid-stride kernel of 256 threads over `items`
static unsigned stream_grid(size_t items) {
    return (unsigned)std::max<size_t>(1, std::min<size_t>((items + 255) / 256, (size_t)num_cus() * 16));
}
// ... and its launch on `st`; a site that picks between two instantiations of a kernel does so before it calls
template <typename K, typename... Args>
static int stream_launch(K kernel, size_t items, hipStream_t st, const Args&... args) {
    hipLaunchKernelGGL(kernel, dim3(stream_grid(items)), dim3(256), 0, st, args...);
    PF_CHECK(hipGetLastError());
    return 0;
}

// `batch` rows through the buffer of `st` in `pool`, chunk_rows at a time: body(X, first row, rows) enqueues one chunk and returns 0 or
// an error.  pool.mu is held until the last chunk is enqueued; `what` names the buffer in the capture refusal ("the frame matrix").
template <typename X, class Body>
static int chunked_scratch(StreamScratch& pool, hipStream_t st, size_t batch, size_t row_bytes, const char* what, Body&& body) {
    const size_t chunk = chunk_rows(batch, row_bytes);
    std::lock_guard<std::mutex> lk(pool.mu);
    void* p = nullptr;
    if (int rc = scratch_buffer(pool, st, chunk * row_bytes, what, &p)) return rc;
    for (size_t v0 = 0; v0 < batch; v0 += chunk)
        if (int rc = body(static_cast<X*>(p), v0, std::min(batch - v0, chunk))) return rc;
    return 0;
}

template <typename T, int MODE>
static int launch_rows(const T* src, size_t src_stride, T* dst, size_t dst_stride, size_t count, size_t row, hipStream_t st) {
    const size_t per = MODE == 0 ? row : MODE == 1 ? row / 2 + 1 : row / 2;
    return stream_launch(frames_rows_kernel<T, MODE>, count * per, st, src, src_stride, dst, dst_stride, count, (unsigned)row);
}

// dense spectra rows of X -> out: copied (ordered / internal) or as |X|^2 of a real / complex spectrum
template <typename T>
static int store_rows(bool power, bool real, const T* X, size_t row, T* dst, size_t dst_stride, size_t count, hipStream_t st) {
    if (!power) return launch_rows<T, 0>(X, row, dst, dst_stride, count, row, st);
    return real ? launch_rows<T, 1>(X, row, dst, dst_stride, count, row, st) : launch_rows<T, 2>(X, row, dst, dst_stride, count, row, st);
}

// frames v0 ... v0 + cnt - 1 (numbered i nframes + f) x window -> rows of X: 16 bytes at a time where signal, stride and hop allow
template <typename T>
static int launch_gather(const T* signal, size_t signal_stride, size_t nframes, size_t hop_s, size_t spp, const T* window, T* X, size_t v0,
                         size_t cnt, size_t row, hipStream_t st) {
    constexpr int U = 16 / (int)sizeof(T);
    const bool wide = aligned16(signal) && signal_stride % U == 0 && hop_s % U == 0;
    return stream_launch(wide ? frames_gather_kernel<T, U> : frames_gather_kernel<T, 1>, wide ? cnt * row / U : cnt * row, st, signal, signal_stride,
                         nframes, hop_s, (int)spp, window, X, v0, cnt, (unsigned)row);
}

// ------------------------------------------------------------------------------------------------ analysis (frames, pfb, psd)
struct FrameDims { bool real; size_t spp, N, row, out_row; };   // out_row: scalars of one output row (|X|^2: N/2 + 1 real, N complex)
static FrameDims frame_dims(const Setup* s, int output) {
    const bool real = s->transform == PFFFT_REAL;
    const size_t N = (size_t)s->N;
    return {real, real ? (size_t)1 : 2, N, s->vec_scalars, output == FR_POWER ? (real ? N / 2 + 1 : N) : s->vec_scalars};
}

// What the three analysis entries check and derive alike, in their order; `prefix` ("frames: ") opens every text.  `taps`: the filter
// bank's, with its prototype (NULL: frames of N samples).  `navg`: the PSD entry's, 0 read as nframes.  Returns ARGS_EMPTY for a call
// without frames (the entry returns 0), else 0 or the refusal; signal_stride and out_stride come back normalised.
constexpr int ARGS_EMPTY = -1;
struct AnalysisArgs : FrameDims { size_t hop_s, batch; };
template <typename T>
static int analysis_args(const char* prefix, const Setup* s, const T* signal, size_t* signal_stride, size_t nsignals, size_t nframes,
                         size_t hop, const T* out, size_t* out_stride, int output, AnalysisArgs* a, const size_t* taps = nullptr,
                         const T* prototype = nullptr, size_t* navg = nullptr) {
    if (int rc = check_setup<T>(s)) return rc;
    if (hop == 0) return bad_in(prefix, "hop == 0");
    if (taps && *taps == 0) return bad_in(prefix, "taps == 0");
    if (taps && !prototype) return bad_in(prefix, "NULL prototype");
    if (output != FR_INTERNAL && output != FR_ORDERED && output != FR_POWER) return bad_in(prefix, "unknown output");
    if (nsignals == 0 || nframes == 0) return ARGS_EMPTY;
    if (navg) {
        if (*navg == 0) *navg = nframes;
        if (nframes % *navg) return bad_in(prefix, "nframes is no multiple of navg");
    }
    static_cast<FrameDims&>(*a) = frame_dims(s, output);
    if (*out_stride == 0) *out_stride = a->out_row;
    if (*out_stride < a->out_row) return bad_in(prefix, "out_stride smaller than one output row");
    const size_t sig_scalars = ((nframes - 1) * hop + (taps ? *taps : 1) * a->N) * a->spp;
    if (nsignals > 1 && *signal_stride < sig_scalars) return bad_in(prefix, "signal_stride smaller than one signal's samples");
    if (!signal || !out) return bad_in(prefix, "NULL signal / out");
    a->hop_s = hop * a->spp;
    a->batch = nsignals * nframes;
    if (nsignals == 1) *signal_stride = 0;   // (one signal: the stride is not read)
    return 0;
}

// The composed analysis: head(X, first frame, frames) fills rows of the frame matrix (chunks of at most SCRATCH_CAP_BYTES), then
// transform_batch, then rows -> out where `out` is not the dense spectrum.
template <typename T, class Head>
static int analysis_composed(Setup* s, const AnalysisArgs& a, T* out, size_t out_stride, int output, hipStream_t st, Head&& head) {
    const bool direct = output != FR_POWER && out_stride == a.row;
    return chunked_scratch<T>(s->frames, st, a.batch, a.row * sizeof(T), "the frame matrix", [&](T* X, size_t v0, size_t cnt) {
        if (int rc = head(X, v0, cnt)) return rc;
        T* dst = out + v0 * out_stride;
        if (int rc = transform_batch_any(s, X, direct ? dst : X, cnt, PFFFT_FORWARD, output == FR_INTERNAL ? 0 : 1, st)) return rc;
        return direct ? 0 : store_rows<T>(output == FR_POWER, a.real, X, a.row, dst, out_stride, cnt, st);
    });
}

// ------------------------------------------------------------------------------------------------ synthesis (frames, pfb)
// spectra rows r0 ... r0 + cnt - 1 -> backward-transformed dense rows in X
template <typename T>
static int frames_backward(Setup* s, const T* spectra, size_t spectra_stride, size_t r0, size_t cnt, T* X, int ordered, hipStream_t st) {
    const size_t row = s->vec_scalars;
    const T* src = spectra + r0 * spectra_stride;
    if (spectra_stride != row) {
        int rc = launch_rows<T, 0>(src, spectra_stride, X, row, cnt, row, st);
        if (rc) return rc;
        src = X;
    }
    return transform_batch_any(s, src, X, cnt, PFFFT_BACKWARD, ordered ? 1 : 0, st);
}

// Checked spectra of frames that span `span` samples -> signals: every frame at once where the batch fits under the cap, else by
// synth_plan.  gather(X, first frame in X, frame pitch of a signal in X, frames end, signal, signal_stride, signals, first sample, samples
// end) launches the entry's overlap-add of the rows of X on `st`.
template <typename T, class Gather>
static int synthesis_runs(Setup* s, const T* spectra, size_t spectra_stride, size_t nsignals, size_t nframes, size_t hop, size_t span,
                          size_t min_run, int ordered, T* signal, size_t signal_stride, hipStream_t st, Gather&& gather) {
    s = for_device(s);
    int rc = ensure_device_any(s, st);
    if (rc) return rc;
    const size_t row = s->vec_scalars, samples = (nframes - 1) * hop + span, batch = nsignals * nframes, cap = cap_rows(row * sizeof(T));
    std::lock_guard<std::mutex> lk(s->frames.mu);
    void* buf = nullptr;
    if (batch <= cap) {   // every frame at once, one gather
        if ((rc = scratch_buffer(s->frames, st, batch * row * sizeof(T), "the frame matrix", &buf))) return rc;
        if ((rc = frames_backward<T>(s, spectra, spectra_stride, 0, batch, (T*)buf, ordered, st))) return rc;
        return gather((const T*)buf, 0, nframes, nframes, signal, signal_stride, nsignals, 0, samples);
    }
    const size_t reach = synth_reach(span, hop);
    const RunPlan p = synth_plan(nframes, cap, reach, min_run);
    if ((rc = scratch_buffer(s->frames, st, p.buffer_rows * row * sizeof(T), "the frame matrix", &buf))) return rc;
    for (size_t i = 0; i < nsignals; ++i)
        for (size_t fa = 0; fa < nframes; fa += p.run) {
            const size_t fb = std::min(nframes, fa + p.run), f0 = fa > reach ? fa - reach : 0;
            if ((rc = frames_backward<T>(s, spectra, spectra_stride, i * nframes + f0, fb - f0, (T*)buf, ordered, st))) return rc;
            if ((rc = gather((const T*)buf, f0, 0, fb, signal + i * signal_stride, 0, 1, fa * hop, fb == nframes ? samples : fb * hop))) return rc;
        }
    return 0;
}

// ------------------------------------------------------------------------------------------------ averages (psd, csd)
// The run walk of avg_plan.  Takes the partial buffer of `st` (Setup::psd, where rpg > 1) and then the frame matrix (Setup::frames, where
// composed), always in this order, and hands the runs of each pass to fused(dst, dstride, first output row, runs, scale) or, in chunks, to
// composed(X, first run, runs, first frame, frames, dst, dstride, scale): a run stores into `out` with the scaling (rpg == 1) or into its
// partial row, which reduce(part, rows, out rows) sums after the pass.  The callables enqueue on `st` and return 0 or an error.
// part_row, frame_row: the scalars behind the plan's two byte counts (a partial row; a frame row times the frame sets).
template <typename T, class Fused, class Composed, class Reduce>
static int averaged_runs(Setup* s, hipStream_t st, const AvgPlan& p, size_t part_row, size_t frame_row, T* out, size_t out_stride, T scaling,
                         Fused&& fused, Composed&& composed, Reduce&& reduce) {
    const size_t rpg = p.rpg;
    std::unique_lock<std::mutex> lkp(s->psd.mu, std::defer_lock), lkf(s->frames.mu, std::defer_lock);
    void *part = nullptr, *X = nullptr;
    if (rpg > 1) {
        lkp.lock();
        if (int rc = scratch_buffer(s->psd, st, p.part_rows * part_row * sizeof(T), "the partial buffer", &part)) return rc;
    }
    if (!p.fused) {
        lkf.lock();
        if (int rc = scratch_buffer(s->frames, st, p.set_rows * frame_row * sizeof(T), "the frame matrix", &X)) return rc;
    }
    for (size_t v0 = 0; v0 < p.V; v0 += p.vstep) {
        const size_t rows = std::min(p.V - v0, p.vstep), ra = v0 * rpg, rb = (v0 + rows) * rpg;
        T* dst = rpg == 1 ? out + v0 * out_stride : (T*)part;
        const size_t dstride = rpg == 1 ? out_stride : part_row;
        const T scale = rpg == 1 ? scaling : (T)1;
        if (p.fused) {
            if (int rc = fused(dst, dstride, v0, rb - ra, scale)) return rc;
        } else {
            for (size_t r = ra; r < rb; r += p.crun) {
                const size_t cnt = std::min(rb - r, p.crun), fa = first_frame(r, p.navg, rpg), nfr = first_frame(r + cnt, p.navg, rpg) - fa;
                if (int rc = composed((T*)X, r, cnt, fa, nfr, dst + (r - ra) * dstride, dstride, scale)) return rc;
            }
        }
        if (rpg > 1)
            if (int rc = reduce((T*)part, rows, out + v0 * out_stride)) return rc;
    }
    return 0;
}

// What the fused routes of both entries ask of a call whose pointers are 16-byte aligned: the entry's selector pair and test of the setup,
// 16-byte loads of every frame (hop, strides: multiples of 4 scalars), an average's frames counted in 32 bits, fused under no selector.
template <class Fusable>
static bool averaged_route_fused(const AbSel& sel, AbValue composed, AbValue fused, Fusable&& fusable, size_t hop, size_t stride_a, size_t stride_b,
                                 size_t navg, bool by_default) {
    if (hop % 4 || stride_a % 4 || stride_b % 4 || navg > 0xffffffffull) return false;
    return fused_selected(sel, composed, fused, fusable(), by_default);
}

// the setup a `*_route` export answers for; NULL: it answers ""
inline const Setup* route_setup(const void* setup, size_t hop) {
    const Setup* s = static_cast<const Setup*>(setup);
    return s && s->magic == MAGIC && hop != 0 ? s : nullptr;
}

// ------------------------------------------------------------------------------------------------ the framed register-tiled configuration
template <class C> struct CfgTag { typedef C type; };

// A kernel that frames, folds or accumulates around the register-tiled transform equals transform_batch bit for bit only on the
// configuration transform_batch runs on for the same (direction, layout), so that is read from the setup's stored route `r`: real float on
// TiledPick C512 / C1024 / C2048 (N = 1024 / 2048 / 4096).  visit(CfgTag<C>()) and true, or false: no such kernel.
template <class Visit>
static bool visit_tiled_cfg(const Setup* s, const Route& r, Visit&& visit) {
    if (s->is_double || s->transform != PFFFT_REAL || s->kernel != K_TILED || r.fam != FAM_TILED) return false;
    const std::string cfg = r.tiled.cfg;
    if (s->n == 512 && cfg == "TiledPick::C512") { visit(CfgTag<TiledPick<float>::C512>()); return true; }
    if (s->n == 1024 && cfg == "TiledPick::C1024") { visit(CfgTag<TiledPick<float>::C1024>()); return true; }
    if (s->n == 2048 && cfg == "TiledPick::C2048") { visit(CfgTag<TiledPick<float>::C2048>()); return true; }
    return false;
}

// The complex twin: complex float on TiledPick C256 / C512 (N = 256 / 512), the configurations the type-IV cosine kernel of fft_mdct.h
// is built on (M = 512 / 1024).
template <class Visit>
static bool visit_tiled_cfg_complex(const Setup* s, const Route& r, Visit&& visit) {
    if (s->is_double || s->transform != PFFFT_COMPLEX || s->kernel != K_TILED || r.fam != FAM_TILED) return false;
    const std::string cfg = r.tiled.cfg;
    if (s->n == 256 && cfg == "TiledPick::C256") { visit(CfgTag<TiledPick<float>::C256>()); return true; }
    if (s->n == 512 && cfg == "TiledPick::C512") { visit(CfgTag<TiledPick<float>::C512>()); return true; }
    return false;
}

// ------------------------------------------------------------------------------------------------ handles that own an inner setup
// Base of every derived handle: the magic word first, the owned PFFFT_Setup / PFFFTD_Setup objects.  `inner` is the first one (new_inner, which
// fixes the precision); a handle that needs more asks add_inner and keeps the pointers it wants.  drop_inner destroys them all, in the
// order they were created.  A handle type H names itself in H::KIND for the refusal text.
template <uint32_t MAGIC_>
struct InnerOwner {
    static constexpr uint32_t HANDLE_MAGIC = MAGIC_;
    uint32_t magic = MAGIC_;
    int is_double = 0;
    Setup* inner = nullptr;
    std::vector<Setup*> owned;
    ~InnerOwner() { drop_inner(); }
    Setup* add_inner(int len, int transform) {
        Setup* s = is_double ? static_cast<Setup*>(pffftd_new_setup(len, (pffft_transform_t)transform))
                             : static_cast<Setup*>(pffft_new_setup(len, (pffft_transform_t)transform));
        if (s) owned.push_back(s);
        return s;
    }
    bool new_inner(int len, int transform, int dbl) {
        is_double = dbl;
        return (inner = add_inner(len, transform)) != nullptr;
    }
    void drop_inner() {
        for (Setup* s : owned) {
            if (is_double) pffftd_destroy_setup(static_cast<PFFFTD_Setup*>(s));
            else pffft_destroy_setup(static_cast<PFFFT_Setup*>(s));
        }
        owned.clear();
        inner = nullptr;
    }
};

// `inner` with its tables on the calling thread's device, for a handle that serves one device: where for_device would answer with a
// replica, the handle's own tables are on another device and the call is refused
inline int inner_on_device(Setup* inner, hipStream_t st) {
    if (for_device(inner) != inner) return bad("this setup holds its tables on another device", hipErrorInvalidDevice);
    return ensure_device_any(inner, st);
}

// The PUBLIC entries on an inner setup of the scalar type T (they validate and resolve the device: transform_batch_any and its kin do not)
template <typename T>
static int inner_transform_batch(Setup* inner, const T* in, T* out, size_t batch, int dir, int ordered, hipStream_t st) {
    if constexpr (sizeof(T) == 8)
        return pffftd_hip_transform_batch(static_cast<PFFFTD_Setup*>(inner), in, out, batch, (pffft_direction_t)dir, ordered, st);
    else
        return pffft_hip_transform_batch(static_cast<PFFFT_Setup*>(inner), in, out, batch, (pffft_direction_t)dir, ordered, st);
}
template <typename T>
static int inner_convolve_batch(Setup* inner, const T* in, const T* H, T* out, T scaling, size_t batch, hipStream_t st) {   // one H, no accumulation
    if constexpr (sizeof(T) == 8)
        return pffftd_hip_convolve_batch(static_cast<PFFFTD_Setup*>(inner), in, H, out, scaling, batch, 0, 1, st);
    else
        return pffft_hip_convolve_batch(static_cast<PFFFT_Setup*>(inner), in, H, out, scaling, batch, 0, 1, st);
}
template <typename T>
static int inner_zreorder_batch(Setup* inner, const T* in, T* out, size_t batch, int dir, hipStream_t st) {
    if constexpr (sizeof(T) == 8)
        return pffftd_hip_zreorder_batch(static_cast<PFFFTD_Setup*>(inner), in, out, batch, (pffft_direction_t)dir, st);
    else
        return pffft_hip_zreorder_batch(static_cast<PFFFT_Setup*>(inner), in, out, batch, (pffft_direction_t)dir, st);
}

template <class H>
static H* checked_handle(const void* p) {
    const H* h = static_cast<const H*>(p);
    return h && h->magic == H::HANDLE_MAGIC ? const_cast<H*>(h) : nullptr;
}
// ... of the scalar type T, or NULL with the refusal text set: the entry returns hipErrorInvalidHandle
template <class H, typename T>
static H* typed_handle(const void* p) {
    H* h = checked_handle<H>(p);
    if (h && h->is_double == (sizeof(T) == 8)) return h;
    g_last_error = std::string("pffft_hip: bad ") + H::KIND + " setup handle";
    return nullptr;
}
template <class H>
static void destroy_handle(void* p) {
    H* h = checked_handle<H>(p);
    if (!h) return;
    h->magic = 0;
    h->drop_inner();   // (before the handle's own tables and scratch go)
    delete h;
}

// A handle that serves ONE device, like PFFASTCONV_Setup: the first call binds it to the current device and builds its tables with
// build() (allocates and synchronises: not during a stream capture); a call from a thread whose current device is another one is refused.
struct DeviceBinding {
    std::mutex mu;   // guards the lazy tables
    bool ready = false;
    int device = -1;
};
template <class Build>
static int bind_device_once(DeviceBinding& b, const char* prefix, hipStream_t st, Build&& build) {
    int dev = -1;
    PF_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(b.mu);
    if (b.ready)
        return b.device == dev ? 0 : bad_in(prefix, "this setup holds its tables on another device (one setup serves one device)", hipErrorInvalidDevice);
    if (stream_capturing(st))
        return bad_in(prefix, "the tables of this setup would have to be built during graph capture: run the call once before capturing",
                      hipErrorStreamCaptureUnsupported);
    if (int rc = build()) return rc;
    b.device = dev;
    b.ready = true;
    return 0;
}

}  // namespace pf
