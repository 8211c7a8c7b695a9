// The LZ77 stage of the PNG encoder (opt-in; png.hip's literal-only entries are untouched): the filtered stream of a frame
// (filter type 0 on every row: H rows of 1 + rb bytes, rb = W * channels, L bytes in all) is cut into literals and
// (length, distance) matches and written as ONE final dynamic-Huffman deflate block with both alphabets.
//
// THE TOKEN RULE.  The tokens are a function of the stream alone (tests/helpers/png_lz_ref.py restates it without threads):
//   segment     positions k * 1024 .. k * 1024 + 1023, cut at L; its LANE is k mod 16
//   key(q)      ((S[q] | S[q+1] << 8 | S[q+2] << 16) * 0x9E3779B1 mod 2^32) >> 23, defined for q + 3 <= L (9 bits)
//   candidates  of position p, in this order:
//                 distance 1; c, 2c .. 8c (c = channels); rb + 1 (the pixel above);
//                 the LANE candidate: p - q for the largest q with q + 3 <= L, q's segment on the same lane as p's,
//                   q < 64 * (p / 64) and key(q) == key(p);
//                 the NEIGHBOUR candidate: p - q for the largest q of the segment before p's with q + 3 <= L and
//                   key(q) == key(p)
//               (the last two need p + 3 <= L; each is that ONE q, whatever its distance turns out to be)
//   length      of a candidate d with 1 <= d <= min(p, 32768): the number of i < min(258, segment end - p) with
//               S[p + i] == S[p - d + i], counted from i = 0 without a gap (the source may overlap the target and may lie
//               in earlier segments and tiles; no match runs past its segment's end).  The candidate COUNTS if the length
//               is >= 4, or 3 with d <= 1024 (a far three-byte match costs more bits than three literals)
//   match(p)    the counting candidate of the greatest length, the first in the order above among equals
//   parse       greedy from the start of every segment: a match where match(p) exists (p += length), else a literal
//
// One workgroup of 16 waves per frame walks the stream in tiles of 16 segments; wave w owns segment w of every tile.  LDS
// (about 150 KiB of the CU's 160): a ring of three tiles of stream bytes (the tile and the 32,768 bytes before it), a LANE
// table per wave (512 x uint32, position + 1, never cleared: it is the wave's own history), 17 NEIGHBOUR tables (512 x
// uint16, offset + 1; segment g uses table g mod 17, so segment g - 1's outlives the tile change), and the match of every
// position of the tile (length: 1 byte, distance: 2 bytes).  Per tile:
//   stage      coalesced byte loads into the ring (+ the two bytes behind the tile, for the last keys)
//   pass A     every wave keys its segment in 16 steps of 64 consecutive positions and fills its NEIGHBOUR table; lanes of a
//              step that share a key store until the largest offset stands (offsets only grow from step to step)
//   pass B     the same 16 steps: a step LOOKS UP the wave's LANE table and the previous segment's NEIGHBOUR table, then
//              inserts its own positions with atomicMax -- so a position sees exactly the positions before its step of 64,
//              and the largest one wins whatever the order; then the candidates are measured against the ring
//   walk       a lane owns 16 consecutive positions: it folds their steps into "entered at e, left at x" (registers), the
//              wave hops from chunk to chunk (at most 64 hops, not 1024 steps) and tells every lane where it is entered
//   emit       scan: literal/length and distance counts (LDS atomics; sums do not depend on order).  pack: code bits per
//              lane, wave and workgroup scan, then the bits -- as png.hip's packer: shared first and last words are merged
//              with atomicOr into the zeroed output, every write is checked against the end of the frame's slot
// Nothing is kept between the two entries: the packer recomputes the tokens (no HBM workspace: 0 bytes per frame).
// Registers: both instantiations compile to exactly 128 VGPRs for gfx950, the ceiling for 1024 threads, with no scratch
// (the packer spills some SGPRs); there is no headroom, so anything added to the walk's st[16] / ex[16] arrays goes to scratch.
#include "common.h"
#include "deflate_bits.h"

namespace {

constexpr int LZ_T = 1024;
constexpr int LZ_WAVES = LZ_T / SPNET_WAVE;
constexpr int LZ_SEG = 1024;
constexpr int LZ_TILE = LZ_WAVES * LZ_SEG;
constexpr int LZ_RING = 3 * LZ_TILE;
constexpr int LZ_KEY_BITS = 9;
constexpr int LZ_KEYS = 1 << LZ_KEY_BITS;
constexpr int LZ_NB_TABLES = LZ_WAVES + 1;
constexpr int LZ_NLL = 286;
constexpr int LZ_ND = 30;
constexpr int LZ_NSYM = LZ_NLL + LZ_ND;
constexpr int LZ_HDR_WORDS = 72;            // 2304 bits >= 3 + 14 + 19 * 3 + 316 * 7 = 2286
constexpr int LZ_WINDOW = 32768;
constexpr int LZ_MAX_LEN = 258;
constexpr int LZ_NEAR = 1024;
constexpr int LZ_PIXEL_MULTIPLES = 8;

struct LzArgs {
  const unsigned char* src;
  const uint32_t* lcodes;
  const uint32_t* dcodes;
  const uint32_t* header;
  const int* header_bits;
  const long long* offsets;
  const uint32_t* adler;
  uint32_t* out;
  long out_bytes;
  uint32_t* lhist;
  uint32_t* dhist;
  int H, rb, channels;
};

// RFC 1951 section 3.2.5: symbol, number of extra bits and their value of a length 3 .. 258 / a distance 1 .. 32768
__device__ __forceinline__ void lz_length_symbol(int len, unsigned& sym, unsigned& eb, unsigned& ev) {
  const unsigned v = (unsigned)(len - 3);
  if (v < 8u) { sym = 257u + v; eb = 0u; ev = 0u; return; }
  if (v == 255u) { sym = 285u; eb = 0u; ev = 0u; return; }
  const unsigned k = 31u - (unsigned)__clz((int)v);
  const unsigned r = v - (1u << k);
  eb = k - 2u;
  sym = 265u + 4u * (eb - 1u) + (r >> eb);
  ev = r & ((1u << eb) - 1u);
}

__device__ __forceinline__ void lz_distance_symbol(int dist, unsigned& sym, unsigned& eb, unsigned& ev) {
  const unsigned v = (unsigned)(dist - 1);
  if (v < 4u) { sym = v; eb = 0u; ev = 0u; return; }
  const unsigned k = 31u - (unsigned)__clz((int)v);
  eb = k - 1u;
  sym = 2u * k + ((v >> (k - 1u)) & 1u);
  ev = v & ((1u << eb) - 1u);
}

template <bool PACK>
__global__ __launch_bounds__(LZ_T) void png_lz_kernel(const LzArgs a) {
  __shared__ __align__(16) unsigned char s_ring[LZ_RING];
  __shared__ uint32_t s_lane[LZ_WAVES][LZ_KEYS];
  __shared__ unsigned short s_nb[LZ_NB_TABLES][LZ_KEYS];
  __shared__ unsigned short s_dist[LZ_TILE];              // pass A: the key; pass B on: the match's distance, 0 = none
  __shared__ unsigned char s_len[LZ_TILE];                // the match's length - 3
  __shared__ uint32_t s_tab[LZ_NSYM];                     // scan: the counts; pack: length << 16 | code, first bit in bit 0
  __shared__ unsigned s_wtot[LZ_WAVES];
  __shared__ unsigned char s_look[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long n = blockIdx.x;

  long long o0 = 0, o1 = 0;
  unsigned long long limit = 0, carry = 0;
  uint32_t* out = a.out;
  if (PACK) {
    if (a.header_bits[n] < 0) return;                                      // (uniform) a frame the literal packer writes
    o0 = a.offsets[n];
    o1 = a.offsets[n + 1];
    if (o0 < 0 || o1 < o0 || o1 > (long long)a.out_bytes) return;          // (uniform) a slot outside the buffer
    limit = (unsigned long long)o1 * 8ull;
    for (int s = tid; s < LZ_NSYM; s += LZ_T) {
      const uint32_t c = (s < LZ_NLL) ? a.lcodes[n * LZ_NLL + s] : a.dcodes[n * LZ_ND + (s - LZ_NLL)];
      s_tab[s] = code_table_entry(c);
    }
    const int hb = min(a.header_bits[n], LZ_HDR_WORDS * 32);
    carry = write_stream_head<LZ_HDR_WORDS>(out, o0, limit, a.header + n * LZ_HDR_WORDS, hb, tid);
  } else {
    for (int s = tid; s < LZ_NSYM; s += LZ_T) s_tab[s] = 0u;
  }
  for (int i = tid; i < LZ_WAVES * LZ_KEYS; i += LZ_T) (&s_lane[0][0])[i] = 0u;

  const int rb = a.rb, rb1 = rb + 1, ch = a.channels;
  const long nsrc = (long)a.H * rb, L = nsrc + a.H;
  const unsigned char* src = a.src + n * nsrc;
  RowCursor<LZ_T> cur(tid, rb1);                          // stream index tid + 1024 m of the m-th staging step
  const int wbase = wave * LZ_SEG;
  __syncthreads();

  long tile = 0;
  for (long t = 0; tile < L; ++t, tile += LZ_TILE) {
    const int sbase = (int)(t % 3) * LZ_TILE;
    // ---- stage
#pragma unroll
    for (int k = 0; k < LZ_TILE / LZ_T; ++k) {
      const long i = tile + (long)k * LZ_T + tid;
      s_ring[sbase + k * LZ_T + tid] = stream_byte(src, rb, cur, i < L);
      cur.step();
    }
    if (tid < 2) {
      const long i = tile + LZ_TILE + tid;
      unsigned char d = 0;
      if (i < L) {
        const long r = i / rb1;
        const int c = (int)(i - r * rb1);
        if (c > 0) d = src[r * rb + (c - 1)];
      }
      s_look[tid] = d;
    }
    __syncthreads();

    const long seg0 = tile + wbase;                                        // the wave's segment
    const int seglen = (int)min(max(L - seg0, 0L), (long)LZ_SEG);
    const long g = t * LZ_WAVES + wave;
    const unsigned char* seg = s_ring + sbase + wbase;
    // ---- pass A: keys, and the segment's NEIGHBOUR table
    {
      volatile unsigned short* nb = s_nb[g % LZ_NB_TABLES];
      for (int i = lane; i < LZ_KEYS; i += SPNET_WAVE) nb[i] = 0;
      __builtin_amdgcn_wave_barrier();
      for (int k = 0; k < LZ_SEG / SPNET_WAVE; ++k) {
        const int o = k * SPNET_WAVE + lane;
        const bool keyed = seg0 + o + 3 <= L;
        unsigned key = 0;
        if (keyed) {
          const unsigned b0 = seg[o];
          const unsigned b1 = (wbase + o + 1 < LZ_TILE) ? seg[o + 1] : s_look[wbase + o + 1 - LZ_TILE];
          const unsigned b2 = (wbase + o + 2 < LZ_TILE) ? seg[o + 2] : s_look[wbase + o + 2 - LZ_TILE];
          key = ((b0 | (b1 << 8) | (b2 << 16)) * 0x9E3779B1u) >> (32 - LZ_KEY_BITS);
        }
        s_dist[wbase + o] = (unsigned short)key;
        bool pending = keyed;
        while (__any(pending)) {
          if (pending) nb[key] = (unsigned short)(o + 1);
          __builtin_amdgcn_wave_barrier();
          if (pending) pending = nb[key] < (unsigned short)(o + 1);
          __builtin_amdgcn_wave_barrier();
        }
      }
    }
    __syncthreads();

    // ---- pass B: the match of every position
    {
      volatile uint32_t* mine = s_lane[wave];
      const volatile unsigned short* prev = s_nb[(g + LZ_NB_TABLES - 1) % LZ_NB_TABLES];
      for (int k = 0; k < LZ_SEG / SPNET_WAVE; ++k) {
        const int o = k * SPNET_WAVE + lane;
        const long p = seg0 + o;
        const bool keyed = p + 3 <= L;
        const unsigned key = s_dist[wbase + o];
        uint32_t e_lane = 0, e_prev = 0;
        if (keyed) {
          e_lane = mine[key];
          if (g > 0) e_prev = prev[key];
        }
        __builtin_amdgcn_wave_barrier();
        if (keyed) atomicMax((uint32_t*)&mine[key], (uint32_t)(p + 1));
        __builtin_amdgcn_wave_barrier();

        const int cap = min(LZ_MAX_LEN, seglen - o);
        const int dmax = (int)min(p, (long)LZ_WINDOW);
        const int ti = sbase + wbase + o;                                  // the target in the ring: never wraps
        int best = 0, best_d = 0;
        auto offer = [&](long dl) {
          if (dl < 1 || dl > dmax || best >= cap) return;
          const int d = (int)dl;
          int si = ti - d;
          if (si < 0) si += LZ_RING;
          if (best > 0) {                                                  // only a longer one replaces the best so far
            int sj = si + best;
            if (sj >= LZ_RING) sj -= LZ_RING;
            if (s_ring[ti + best] != s_ring[sj]) return;
          }
          int m = 0;
          while (m < cap) {
            int sj = si + m;
            if (sj >= LZ_RING) sj -= LZ_RING;
            if (s_ring[ti + m] != s_ring[sj]) break;
            ++m;
          }
          if (m > best && (m >= 4 || (m == 3 && d <= LZ_NEAR))) { best = m; best_d = d; }
        };
        if (cap >= 3) {
          offer(1);
          for (int j = 1; j <= LZ_PIXEL_MULTIPLES; ++j) offer(ch * j);
          offer(rb1);
          if (e_lane) offer(p - (long)(e_lane - 1u));
          if (e_prev) offer((long)o + LZ_SEG - (long)(e_prev - 1u));
        }
        s_dist[wbase + o] = (unsigned short)best_d;
        s_len[wbase + o] = (unsigned char)(best ? best - 3 : 0);
      }
    }
    __syncthreads();

    // ---- walk: which positions start a token
    int st[16], ex[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int r = wbase + lane * 16 + e;
      st[e] = s_dist[r] ? (int)s_len[r] + 3 : 1;
    }
#pragma unroll
    for (int e = 15; e >= 0; --e) {                                        // entered at e, the chunk is left at ex[e] >= 16
      const int x = e + st[e];
      int v = x;
#pragma unroll
      for (int j = e + 1; j < 16; ++j) v = (x == j) ? ex[j] : v;
      ex[e] = v;
    }
    int entry = 99;
    for (int pos = 0; pos < seglen;) {                                     // (uniform in the wave)
      const int c = pos >> 4, e = pos & 15;
      int v = ex[0];
#pragma unroll
      for (int j = 1; j < 16; ++j) v = (e == j) ? ex[j] : v;
      const int x = __shfl(v, c, SPNET_WAVE);
      if (lane == c) entry = e;
      pos = __builtin_amdgcn_readfirstlane((c << 4) + x);
    }

    // ---- emit
    auto for_tokens = [&](auto&& f) {
      int nx = entry;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        if (e == nx) {
          const int o = lane * 16 + e;
          if (o < seglen) f(o, st[e]);
          nx = e + st[e];
        }
      }
    };
    if (!PACK) {
      for_tokens([&](int o, int step) {
        const int dist = s_dist[wbase + o];
        if (dist == 0) {
          atomicAdd(&s_tab[seg[o]], 1u);
        } else {
          unsigned sym, eb, ev;
          lz_length_symbol(step, sym, eb, ev);
          atomicAdd(&s_tab[sym], 1u);
          lz_distance_symbol(dist, sym, eb, ev);
          atomicAdd(&s_tab[LZ_NLL + sym], 1u);
        }
      });
    } else {
      // a token as two fields of at most 20 and 28 bits: (literal or length code + length extra), (distance code + extra)
      auto fields = [&](int o, int step, uint32_t& f0, unsigned& n0, uint32_t& f1, unsigned& n1) {
        const int dist = s_dist[wbase + o];
        if (dist == 0) {
          const uint32_t c = s_tab[seg[o]];
          f0 = c & 0xffffu; n0 = c >> 16; f1 = 0u; n1 = 0u;
        } else {
          unsigned sym, eb, ev;
          lz_length_symbol(step, sym, eb, ev);
          uint32_t c = s_tab[sym];
          f0 = (c & 0xffffu) | (ev << (c >> 16)); n0 = (c >> 16) + eb;
          lz_distance_symbol(dist, sym, eb, ev);
          c = s_tab[LZ_NLL + sym];
          f1 = (c & 0xffffu) | (ev << (c >> 16)); n1 = (c >> 16) + eb;
        }
      };
      unsigned bits = 0;
      for_tokens([&](int o, int step) {
        uint32_t f0, f1;
        unsigned n0, n1;
        fields(o, step, f0, n0, f1, n1);
        bits += n0 + n1;
      });
      // (scan, accumulator and tail are written out as in png.hip: as shared functions they change this kernel's code)
      unsigned incl = bits;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const unsigned v = (unsigned)__shfl_up((int)incl, off, 64);
        if (lane >= off) incl += v;
      }
      if (lane == 63) s_wtot[wave] = incl;
      __syncthreads();
      unsigned before = 0, total = 0;
      for (int w = 0; w < LZ_WAVES; ++w) {
        const unsigned v = s_wtot[w];
        before += (w < wave) ? v : 0u;
        total += v;
      }
      const unsigned long long pos = carry + before + (incl - bits);
      if (bits > 0 && pos + bits <= limit) {
        uint32_t* wp = out + (pos >> 5);
        unsigned long long acc = 0;
        unsigned nacc = (unsigned)(pos & 31);                              // the bits below belong to the neighbour
        bool shared = true;                                                // the first word may hold a neighbour's bits
        auto put = [&](uint32_t v, unsigned nb) {                          // nacc < 32 and nb <= 28: at most 59 bits held
          acc |= (unsigned long long)v << nacc;
          nacc += nb;
          if (nacc >= 32u) {
            if (shared) atomicOr(wp, (uint32_t)acc);
            else *wp = (uint32_t)acc;
            shared = false;
            ++wp;
            acc >>= 32;
            nacc -= 32u;
          }
        };
        for_tokens([&](int o, int step) {
          uint32_t f0, f1;
          unsigned n0, n1;
          fields(o, step, f0, n0, f1, n1);
          put(f0, n0);
          put(f1, n1);
        });
        if (nacc > 0u) atomicOr(wp, (uint32_t)acc);
      }
      carry += total;
    }
    __syncthreads();                                       // the ring's next slot, s_look, s_dist and s_wtot are rewritten
  }

  if (!PACK) {
    for (int s = tid; s < LZ_NSYM; s += LZ_T) {
      if (s < LZ_NLL) a.lhist[n * LZ_NLL + s] = s_tab[s] + (s == 256 ? 1u : 0u);      // the end of block, once
      else a.dhist[n * LZ_ND + (s - LZ_NLL)] = s_tab[s];
    }
  } else {
    // end of block, zero bits up to the next byte (the buffer arrives zeroed), Adler-32 most significant byte first
    const uint32_t eob = s_tab[256];
    if (tid == 0 && (eob >> 16)) or_bits(out, carry, limit, eob & 0xffffu, (int)(eob >> 16));
    const unsigned long long tail = ((carry + (eob >> 16) + 7ull) >> 3) * 8ull;
    if (tid >= 64 && tid < 68) {
      const int k = tid - 64;
      or_bits(out, tail + 8ull * k, limit, (a.adler[n] >> (24 - 8 * k)) & 255u, 8);
    }
  }
}

}  // namespace

extern "C" int spnet_png_lz_scan(const unsigned char* src, int N, int H, int W, int channels, uint32_t* lhist, uint32_t* dhist,
                                 void* stream) {
  if (!png_shape_ok(N, H, W, channels) || !src || !lhist || !dhist) return (int)hipErrorInvalidValue;
  if (((uintptr_t)lhist | (uintptr_t)dhist) & 3) return (int)hipErrorInvalidValue;
  if (N == 0) return 0;
  LzArgs a = {};
  a.src = src; a.lhist = lhist; a.dhist = dhist; a.H = H; a.rb = W * channels; a.channels = channels;
  hipLaunchKernelGGL(png_lz_kernel<false>, dim3((unsigned)N), dim3(LZ_T), 0, (hipStream_t)stream, a);
  SPNET_RETURN_LAUNCH_STATUS();
}

extern "C" int spnet_png_lz_pack(const unsigned char* src, int N, int H, int W, int channels, const uint32_t* lcodes,
                                 const uint32_t* dcodes, const uint32_t* header, const int* header_bits,
                                 const long long* offsets, const uint32_t* adler, unsigned char* out, long out_bytes,
                                 void* stream) {
  if (!png_shape_ok(N, H, W, channels) || !src || !lcodes || !dcodes || !header || !header_bits || !offsets || !adler || !out)
    return (int)hipErrorInvalidValue;
  if (out_bytes < 0 || (out_bytes & 3)) return (int)hipErrorInvalidValue;            // whole 32-bit words
  if (((uintptr_t)lcodes | (uintptr_t)dcodes | (uintptr_t)header | (uintptr_t)header_bits | (uintptr_t)adler |
       (uintptr_t)out) & 3)
    return (int)hipErrorInvalidValue;
  if ((uintptr_t)offsets & 7) return (int)hipErrorInvalidValue;
  if (N == 0) return 0;
  LzArgs a = {};
  a.src = src; a.lcodes = lcodes; a.dcodes = dcodes; a.header = header; a.header_bits = header_bits; a.offsets = offsets;
  a.adler = adler; a.out = reinterpret_cast<uint32_t*>(out); a.out_bytes = out_bytes; a.H = H; a.rb = W * channels;
  a.channels = channels;
  hipLaunchKernelGGL(png_lz_kernel<true>, dim3((unsigned)N), dim3(LZ_T), 0, (hipStream_t)stream, a);
  SPNET_RETURN_LAUNCH_STATUS();
}
