// Cosine and sine transforms of types II and III (pffft[d]_hip_dct_transform_batch): the kernels.  Makhoul's algorithm - one real
// transform of the same N = 2n around a permutation and ONE product with a folded table t_k, k = 0 ... n (include/pffft_hip.h):
//   type II   v[m] = x[2m], v[N-1-m] = x[2m+1];  V = real forward transform of v;  z_k = V[k] t_k;
//             X[k] = Re z_k, X[N-k] = -Im z_k (0 < k < n), X[0] = V[0] t_0.x, X[n] = V[n] t_n.x
//   type III  V[k] = (X[k], -X[N-k]) t_k (0 < k < n), V[0] = X[0] t_0.x, V[n] = 2 X[n] t_n.x;  v = unscaled real backward transform of V;
//             y[2m] = v[m], y[2m+1] = v[N-1-m]
//   sine      DST-II(x)[k] = DCT-II((-1)^n x)[N-1-k];  DST-III(X)[n] = (-1)^n DCT-III(reverse X)[n]
//
//   fft_dct_kernel      the FUSED route - the register-tiled real transform of fft_tiled.h between an input and an output round trip
//                       through the transform's own LDS image: 4N bytes read and 4N written per row, one launch.  A kernel of its own
//                       built from the Tiled<> helpers: fft_tiled_kernel keeps its code.  Everything between the permutation and the
//                       table product is the sequence of fft_tiled_kernel<C, DIR, 1>, the product is dct_mul (cxmath.h) on both routes:
//                       the result equals the composed route's bit for bit (tests/test_gpu_dct.py).
//   dct_pre_kernel, dct_post_kernel
//                       the streaming kernels of the COMPOSED route around transform_batch (canonical layout) in a scratch image.
#pragma once
#include "fft_tiled.h"
#include "pf_handout.h"

namespace pf {

enum { DCT_2 = 0, DCT_3 = 1, DST_2 = 2, DST_3 = 3 };   // pffft_hip_dct_kind_t
__host__ __device__ constexpr bool dct_type3(int kind) { return kind == DCT_3 || kind == DST_3; }
__host__ __device__ constexpr bool dct_sine(int kind) { return kind == DST_2 || kind == DST_3; }

// LDS images of fft_dct_kernel.  The packed points z go into the NATURAL image of the transform (phys_nat: the padding the stage-0
// operand reads of the backward canonical loader are conflict-free on).  The real row (N floats: the scattered results of type II, the
// raw input of type III) is LINEAR: lane t of a transform touches k = t + const or const - t in every 4-byte access, i.e. the 32 lanes
// of an access group (ds_read_b32 / ds_write_b32 are served in two halves of 32 lanes on 32 banks) touch 32 consecutive dwords - no
// conflict without padding - and the 16-byte side reads / writes consecutive slots.  A padded block layout (the IBS image of the
// internal layout) would only add address arithmetic.
template <class C, int KIND>
__global__ void __launch_bounds__(C::WG_THREADS, C::OCC)
fft_dct_kernel(const float* in, float* out, unsigned batch, const cx<float>* __restrict__ tab, const cx<float>* __restrict__ twg,
               const cx<float>* __restrict__ twrg, unsigned* ctr) {
    typedef float T;
    typedef cx<T> CX;
    constexpr bool III = dct_type3(KIND), SINE = dct_sine(KIND);
    typedef Tiled<C, III ? BWD : FWD, 1> K;
    typedef typename K::S0 S0;
    typedef typename K::SL SL;
    constexpr int n = C::n, N = 2 * C::n, E = C::E, TPT = C::TPT, NCH = C::NCH;
    constexpr int R0 = K::R0, RL = K::RL, RS = K::RS;
    static_assert(sizeof(typename C::real_t) == 4 && C::VEC == 2 && S0::PAIR && SL::PAIR, "float configurations only");
    static_assert(C::TWMODE == 0 || C::TWMODE == 3, "register twiddles only");
    static_assert(((n / RL) % 64 == 0 && (n / R0) % 64 == 0) || C::PADN == 0, "pad period vs operand stride");
    static_assert(E == 2 * RS, "two butterflies per thread next to the spectrum");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int slot = threadIdx.x / TPT, t = threadIdx.x % TPT;
    CX* img = reinterpret_cast<CX*>(smem_raw) + (size_t)slot * C::IMG;
    T* imgs = reinterpret_cast<T*>(img);
    chunk16* im16 = reinterpret_cast<chunk16*>(img);
    unsigned* s_next = reinterpret_cast<unsigned*>(smem_raw + (size_t)C::T_PER_WG * C::IMG * sizeof(CX));

    typename K::Tw w;
    K::load_tw(w, t, twg, twrg);
    const CX* twt = twg;
    // t_k of the thread's own bins next to the spectrum (they depend on the thread index only); bin 0 packs the two real ends
    CX tk[E];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int d = 0; d < RS; ++d) tk[u * RS + d] = tab[K::template jm<K::SYM_STAGE>(t, u) + d * (n / RS)];
    if (t == 0) tk[0] = mk<T>(tab[0].x, tab[n].x);
    const bool first = (t == 0);

    const bool dyn = ctr != nullptr;
    unsigned g = blockIdx.x;
    unsigned pend = blockIdx.x + gridDim.x;   // hand-out: pf_handout.h
    __syncthreads();
    const size_t last = (size_t)batch - 1;
    auto src_of = [&](size_t tr) -> const T* { return in + (tr < last ? tr : last) * (size_t)N; };
    chunk16 raw[NCH];
    K::load_raw(raw, src_of((size_t)g * C::T_PER_WG + slot), t, false);   // dense chunks in lane order, each once
    for (unsigned it = 0; (size_t)g * C::T_PER_WG < batch; ++it) {
        if (dyn && threadIdx.x == 0) pend = handout_grab(s_next, it, pend, ctr);
        const size_t tr = (size_t)g * C::T_PER_WG + slot;
        const bool active = tr < batch;  // inactive slots recompute the last row and never store
        T* dst = out + (active ? tr : last) * (size_t)N;
        CX v[E];
        int tl = t;
        asm volatile("" : "+v"(tl));

        // ------------------------------------------------------------------ input round trip
        if constexpr (!III) {
            // chunk c = (x0, x1, x2, x3): z[c] = (x0, x2), z[n-1-c] = (x3, x1) (the odd samples negated for the sine form)
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
                const int c = tl + TPT * i;
                const chunk16 r = raw[i];
                lds_st(img + phys_nat<C>(c), mk<T>(r.x, r.z));
                lds_st(img + phys_nat<C>(n - 1 - c), SINE ? mk<T>(-r.w, -r.y) : mk<T>(r.w, r.y));
            }
            K::xsync();
#pragma unroll
            for (int u = 0; u < S0::B; ++u)
#pragma unroll
                for (int q = 0; q < R0; ++q) {
                    const int j = K::template jm<0>(t, u);
                    v[u * R0 + q] = lds_ld_c<0>(img + j + C::PADN * (j >> 6) + K::nat_off(q * (n / R0)));
                }
            K::xsync();
        } else {
            // the raw row into the linear real image; X[k] and X[N-k] of the thread's own stage-0 bins (X[N] = 0; the sine form reads
            // the reversed row), times t_k: the half-complex spectrum the backward transform starts from
#pragma unroll
            for (int i = 0; i < NCH; ++i) im16[t + TPT * i] = raw[i];
            K::xsync();
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int q = 0; q < R0; ++q) {
                    const int k = K::template jm<0>(tl, u) + q * (n / R0);
                    const bool edge = (u == 0 && q == 0) && first;
                    int ia = k, ib = N - k;
                    if (u == 0 && q == 0) { ia = first ? 0 : k; ib = first ? n : N - k; }
                    if (SINE) { ia = N - 1 - ia; ib = N - 1 - ib; }
                    const T a = imgs[ia], b = imgs[ib];
                    v[u * R0 + q] = dct_mul<true>(mk<T>(a, edge ? b : -b), tk[u * R0 + q], edge);
                }
            K::xsync();
            K::pair_regs(v, t, w);   // half-complex spectrum -> packed spectrum, in registers
        }

        // ------------------------------------------------------------------ transform (the sequence of fft_tiled_kernel)
        K::template butterflies<0>(v, t, w, twt);
        if constexpr (C::NS > 1) K::template xwrite<0>(v, t, img);
        __syncthreads();  // publishes s_next; first half of exchange 0
        const unsigned gn = handout_next(dyn, s_next, it, g);
        if constexpr (C::PREFETCH) K::load_raw(raw, src_of((size_t)gn * C::T_PER_WG + slot), t, false);
        if constexpr (C::NS > 1) { K::template xread<0>(v, t, img); K::xsync(); K::template butterflies<1>(v, t, w, twt); }
        if constexpr (C::NS > 2) { K::template xwrite<1>(v, t, img); K::xsync(); K::template xread<1>(v, t, img); K::xsync(); K::template butterflies<2>(v, t, w, twt); }
        if constexpr (C::NS > 3) { K::template xwrite<2>(v, t, img); K::xsync(); K::template xread<2>(v, t, img); K::xsync(); K::template butterflies<3>(v, t, w, twt); }
        if constexpr (C::NS > 4) { K::template xwrite<3>(v, t, img); K::xsync(); K::template xread<3>(v, t, img); K::xsync(); K::template butterflies<4>(v, t, w, twt); }

        // ------------------------------------------------------------------ output round trip
        chunk16* d16 = reinterpret_cast<chunk16*>(dst);
        if constexpr (!III) {
            K::pair_regs(v, t, w);   // v[u RL + d] = bin jm(t, u) + d n/RL of the half-complex spectrum; bin 0 = (DC, Nyquist)
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int d = 0; d < RL; ++d) {
                    const int k = K::template jm<C::NS - 1>(tl, u) + d * (n / RL);
                    const bool edge = (u == 0 && d == 0) && first;
                    const CX z = dct_mul<false>(v[u * RL + d], tk[u * RL + d], edge);
                    int ire = k, iim = N - k;
                    if (u == 0 && d == 0) { ire = first ? 0 : k; iim = first ? n : N - k; }
                    if (SINE) { ire = N - 1 - ire; iim = N - 1 - iim; }
                    imgs[ire] = z.x;
                    imgs[iim] = edge ? z.y : -z.y;
                }
            K::xsync();
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
                const int c = t + TPT * i;
                const chunk16 o = im16[c];
                if (active) __builtin_nontemporal_store(o, d16 + c);
            }
            K::xsync();
        } else {
            // the last stage's operands (the points the plain store of fft_tiled_kernel writes) into the natural image
#pragma unroll
            for (int ii = 0; ii < SL::B / 2; ++ii)
#pragma unroll
                for (int d = 0; d < RL; ++d) {
                    const int P = 2 * (tl + TPT * ii + d * (n / (2 * RL)));
                    lds_st(img + phys_nat<C>(P), v[(2 * ii) * RL + d]);
                    lds_st(img + phys_nat<C>(P + 1), v[(2 * ii + 1) * RL + d]);
                }
            K::xsync();
            // y[4c ... 4c+3] = (v[2c], v[N-1-2c], v[2c+1], v[N-2-2c]) (the odd samples negated for the sine form)
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
                const int c = tl + TPT * i;
                const CX a = lds_ld_c<0>(img + phys_nat<C>(c)), b = lds_ld_c<0>(img + phys_nat<C>(n - 1 - c));
                chunk16 o;
                o.x = a.x; o.y = SINE ? -b.y : b.y; o.z = a.y; o.w = SINE ? -b.x : b.x;
                if (active) __builtin_nontemporal_store(o, d16 + c);
            }
            K::xsync();
        }
        if constexpr (!C::PREFETCH) K::load_raw(raw, src_of((size_t)gn * C::T_PER_WG + slot), t, false);
        g = gn;
    }
    if (dyn && threadIdx.x == 0) handout_rearm(ctr);
}

// LDS of fft_dct_kernel: the images and the counter slot of fft_tiled_kernel (these configurations have no twiddle table)
template <class C> constexpr size_t dct_lds_bytes() { return (size_t)C::T_PER_WG * C::IMG * 2 * sizeof(float) + 16; }

// ------------------------------------------------------------------------------------------------ composed route
// 16-byte (float) / 2 x 16-byte (double) access unit of four scalars, 8- / 16-byte unit of two
template <typename T> struct alignas(16) Quad { T v[4]; };
template <typename T> struct alignas(2 * sizeof(T)) Duo { T v[2]; };

// rows r0 ... of `in` -> the scratch rows the real transform starts from.  Type II: the permutation (one thread per dense chunk of four
// samples, N/4 per row).  Type III: the half-complex spectrum in the canonical layout (one thread per four bins, N/8 per row).
template <typename T, int KIND>
__global__ void dct_pre_kernel(const T* __restrict__ in, T* __restrict__ X, const cx<T>* __restrict__ tab, size_t count, unsigned N) {
    constexpr bool III = dct_type3(KIND), SINE = dct_sine(KIND);
    const unsigned n = N / 2, upr = III ? N / 8 : N / 4;
    const size_t units = count * upr;
    for (size_t x = (size_t)blockIdx.x * blockDim.x + threadIdx.x; x < units; x += (size_t)gridDim.x * blockDim.x) {
        const size_t r = x / upr;
        const unsigned c = (unsigned)(x - r * upr);
        const T* src = in + r * N;
        T* dst = X + r * N;
        if constexpr (!III) {
            const Quad<T> q = *reinterpret_cast<const Quad<T>*>(src + 4 * c);
            Duo<T> a, b;
            a.v[0] = q.v[0]; a.v[1] = q.v[2];
            b.v[0] = SINE ? -q.v[3] : q.v[3]; b.v[1] = SINE ? -q.v[1] : q.v[1];
            *reinterpret_cast<Duo<T>*>(dst + 2 * c) = a;
            *reinterpret_cast<Duo<T>*>(dst + N - 2 - 2 * c) = b;
        } else {
            // A[i] = X'[4c + i], B[i] = X'[N - 4c - 4 + i], e = X'[N - 4c] (X'[N] = 0); X' = X, or the reversed row for the sine form
            const Quad<T> qa = *reinterpret_cast<const Quad<T>*>(src + 4 * c);
            const Quad<T> qb = *reinterpret_cast<const Quad<T>*>(src + N - 4 - 4 * c);
            T A[4], B[4], e = (T)0;
#pragma unroll
            for (int i = 0; i < 4; ++i) { A[i] = SINE ? qb.v[3 - i] : qa.v[i]; B[i] = SINE ? qa.v[3 - i] : qb.v[i]; }
            if (c) e = SINE ? src[4 * c - 1] : src[N - 4 * c];
            const Quad<cx<T>> tq = *reinterpret_cast<const Quad<cx<T>>*>(tab + 4 * c);
            cx<T> V[4];
            V[0] = dct_mul<true>(mk<T>(A[0], -e), tq.v[0], false);
#pragma unroll
            for (int i = 1; i < 4; ++i) V[i] = dct_mul<true>(mk<T>(A[i], -B[4 - i]), tq.v[i], false);
            if (c == 0) V[0] = dct_mul<true>(mk<T>(A[0], SINE ? src[n - 1] : src[n]), mk<T>(tab[0].x, tab[n].x), true);
            Quad<T> o0, o1;
            o0.v[0] = V[0].x; o0.v[1] = V[0].y; o0.v[2] = V[1].x; o0.v[3] = V[1].y;
            o1.v[0] = V[2].x; o1.v[1] = V[2].y; o1.v[2] = V[3].x; o1.v[3] = V[3].y;
            *reinterpret_cast<Quad<T>*>(dst + 8 * c) = o0;
            *reinterpret_cast<Quad<T>*>(dst + 8 * c + 4) = o1;
        }
    }
}

// the transformed scratch rows -> rows of `out`.  Type II: table product and scatter (one thread per four bins k = 4c ... 4c+3 and the
// four mirrored outputs N-4c-4 ... N-4c-1, which take -Im of the bins 4c+1 ... 4c+4: two dense 16-byte stores per precision unit).
// Type III: the inverse permutation (one thread per dense chunk of four outputs).
template <typename T, int KIND>
__global__ void dct_post_kernel(const T* __restrict__ X, T* __restrict__ out, const cx<T>* __restrict__ tab, size_t count, unsigned N) {
    constexpr bool III = dct_type3(KIND), SINE = dct_sine(KIND);
    const unsigned n = N / 2, upr = III ? N / 4 : N / 8;
    const size_t units = count * upr;
    for (size_t x = (size_t)blockIdx.x * blockDim.x + threadIdx.x; x < units; x += (size_t)gridDim.x * blockDim.x) {
        const size_t r = x / upr;
        const unsigned c = (unsigned)(x - r * upr);
        const T* src = X + r * N;
        T* dst = out + r * N;
        if constexpr (III) {
            const Duo<T> a = *reinterpret_cast<const Duo<T>*>(src + 2 * c);
            const Duo<T> b = *reinterpret_cast<const Duo<T>*>(src + N - 2 - 2 * c);
            Quad<T> o;
            o.v[0] = a.v[0]; o.v[1] = SINE ? -b.v[1] : b.v[1]; o.v[2] = a.v[1]; o.v[3] = SINE ? -b.v[0] : b.v[0];
            *reinterpret_cast<Quad<T>*>(dst + 4 * c) = o;
        } else {
            const Quad<T> s0 = *reinterpret_cast<const Quad<T>*>(src + 8 * c);
            const Quad<T> s1 = *reinterpret_cast<const Quad<T>*>(src + 8 * c + 4);
            const bool top = 4 * c + 4 == n;   // bin 4c + 4 is n: V[n] sits in the second scalar of the row
            cx<T> V[5], z[5];
            V[0] = mk<T>(s0.v[0], s0.v[1]); V[1] = mk<T>(s0.v[2], s0.v[3]);
            V[2] = mk<T>(s1.v[0], s1.v[1]); V[3] = mk<T>(s1.v[2], s1.v[3]);
            V[4] = mk<T>((T)0, (T)0);
            if (!top) { const Duo<T> s2 = *reinterpret_cast<const Duo<T>*>(src + 8 * c + 8); V[4] = mk<T>(s2.v[0], s2.v[1]); }
            const Quad<cx<T>> tq = *reinterpret_cast<const Quad<cx<T>>*>(tab + 4 * c);
#pragma unroll
            for (int i = 0; i < 4; ++i) z[i] = dct_mul<false>(V[i], tq.v[i], false);
            z[4] = dct_mul<false>(V[4], tab[4 * c + 4], false);
            Quad<T> lo, up;   // lo[i] = X[4c + i], up[j] = X[N - 4c - 4 + j] of the cosine form
#pragma unroll
            for (int i = 0; i < 4; ++i) { lo.v[i] = z[i].x; up.v[i] = -z[4 - i].y; }
            if (c == 0 || top) {
                const cx<T> e = dct_mul<false>(mk<T>(src[0], src[1]), mk<T>(tab[0].x, tab[n].x), true);
                if (c == 0) lo.v[0] = e.x;
                if (top) up.v[0] = e.y;
            }
            if (SINE) {   // output index N-1-k: the two chunks change places, each reversed
                Quad<T> a, b;
#pragma unroll
                for (int i = 0; i < 4; ++i) { a.v[i] = up.v[3 - i]; b.v[i] = lo.v[3 - i]; }
                lo = a; up = b;
            }
            *reinterpret_cast<Quad<T>*>(dst + 4 * c) = lo;
            *reinterpret_cast<Quad<T>*>(dst + N - 4 - 4 * c) = up;
        }
    }
}

}  // namespace pf
