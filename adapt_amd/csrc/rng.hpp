// rng.hpp — counter-based RNG for the path tracer: Philox-4x32-10 (Salmon et al., SC'11).
//
// Replaces the reference's stateful `ti.random` (third-party Taichi; call sites listed in
// SURVEY.md A.4).  Stream definition (the CPU checker and the golden generator implement the same stream):
//   key     = (global pixel index x*H + y, seed)
//   counter = (sample counter `cnt` of that pixel-sample, draw_index / 4, 0, 0)
//   draw d  = word (d & 3) of that block; floats use the top 24 bits -> [0,1); ints are the raw word
// A path carries only its draw index; the last generated block is cached in registers.
#pragma once
#include "vec.hpp"
#include <stdint.h>
#include <type_traits>

struct Philox {
    uint32_t key0, key1, ctr0;
    uint32_t draw;
    uint32_t blk;        // block index held in c[] (0xffffffff = none)
    uint32_t nblk;       // block index held in n[] (0xffffffff = none): only ever set by rng_open
    uint32_t c[4], n[4];
};

APT_HD void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
#if defined(__HIP_DEVICE_COMPILE__)
    // A stage calls this from several inlined draw sites with the same key.  Left alone, the compiler shares the ten
    // per-round keys (k0 + r * 0x9E3779B9) between the sites and keeps them in ~10 VGPRs for the whole kernel; making the
    // key opaque per call re-derives them with ten adds each time and frees those registers.
    asm volatile("" : "+v"(k0));
#endif
#pragma unroll
    for (int r = 0; r < 10; r++) {
        uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        uint32_t n1 = (uint32_t)p1;
        uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        uint32_t n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

APT_HD void rng_init(Philox& r, uint32_t pixel, uint32_t seed, uint32_t sample, uint32_t draw) {
    r.key0 = pixel; r.key1 = seed; r.ctr0 = sample; r.draw = draw; r.blk = 0xffffffffu; r.nblk = 0xffffffffu;
    r.c[0] = r.c[1] = r.c[2] = r.c[3] = 0u;
    r.n[0] = r.n[1] = r.n[2] = r.n[3] = 0u;
}
APT_HD uint32_t rng_u32(Philox& r) {
    const uint32_t d = r.draw++;
    const uint32_t b = d >> 2;
    const bool step = b != r.blk;
    if (step && b != r.nblk) { philox4x32_10(r.ctr0, b, 0u, 0u, r.key0, r.key1, r.n); r.nblk = b; }      // not opened ahead: generate here
    if (step) { r.c[0] = r.n[0]; r.c[1] = r.n[1]; r.c[2] = r.n[2]; r.c[3] = r.n[3]; r.blk = b; r.nblk = 0xffffffffu; }
    const uint32_t w = d & 3u, c0 = r.c[0], c1 = r.c[1], c2 = r.c[2], c3 = r.c[3];     // select without dynamic register indexing (of VALUES: a conditional over the array's lvalues is a pointer phi, which can keep the block in scratch)
    return (w == 0u) ? c0 : ((w == 1u) ? c1 : ((w == 2u) ? c2 : c3));
}
// For a stage that draws at most five numbers per path: both blocks those draws can touch, generated now, unconditionally.  A generation
// computes every lane's own block in one pass, but left to the draw sites it runs at every site where ANY lane steps into a new block,
// and the lanes of an unsorted queue sit at unrelated offsets of their streams: 3.4 passes per shade on the Cornell box where two
// serve every lane (k_shade, point lights, one light sample: 3.03 -> 2.83 ms per 64 spp).  Stages that draw more keep the lazy
// per-site generation: there the second buffer only costs registers (measured: C3 13.2 -> 14.7 ms with it).
// Used by the class kernels without area lights (k_shade_group, emitter set point + spot) and, with APT_DRAW_WINDOW=0, by the traced
// kernels without area lights; those draw from a DrawWindow (below) otherwise, which generates the second block only when it is read.
APT_HD void rng_open(Philox& r) {
    const uint32_t b = r.draw >> 2;
    philox4x32_10(r.ctr0, b, 0u, 0u, r.key0, r.key1, r.c); r.blk = b;
    philox4x32_10(r.ctr0, b + 1u, 0u, 0u, r.key0, r.key1, r.n); r.nblk = b + 1u;
}
APT_HD float rng_float(Philox& r) { return (float)(rng_u32(r) >> 8) * (1.0f / 16777216.0f); }
APT_HD int32_t rng_int(Philox& r) { return (int32_t)rng_u32(r); }

// The draw window: the same stream for a vertex whose draws are all decided when it is opened - the traced kernels without area lights
// (shade_stage.hpp shade_traced): [roulette] emitter index [emitter index again, on a surface that carries an emitter] direction u1, u2.
// Three to five words from draw index d0 on, so they lie in block d0 / 4 and, for some offsets only, in the next one.  window_open
// generates the first block, tests the roulette on its word, generates the second block only if a surviving lane's LAST word lies in it
// (`any`: the wave's vote - one scalar branch around the pass; on the Cornell box no lane of any wave needs it at bounces 1 and 2), and
// then rotates the words into the three registers the draw sites read by name: `e` for the emitter index (the index that counts - a
// second index draw replaces the first, so both sites read the same register), `u[]` for the direction.  The roulette and the second
// index draw shift the window, not the sites.  After window_open only `draw` is generator state: no key, no counter, no cached block
// and no generation code behind any draw site (Philox's rng_u32 keeps a lazy ten-round pass at every site, which rng_open's callers never
// take and the compiler cannot remove).
#ifndef APT_DRAW_WINDOW
#define APT_DRAW_WINDOW 1
#endif
struct DrawWindow {
    uint32_t draw;       // the path's draw index, advanced by every site as Philox advances it
    uint32_t e, u[2];
    uint32_t rr;         // the roulette's word (read inside window_open only; kept for the host test)
};
APT_HD void rng_init(DrawWindow& w, uint32_t, uint32_t, uint32_t, uint32_t draw) { w.draw = draw; w.e = w.u[0] = w.u[1] = w.rr = 0u; }
APT_HD float window_unit(uint32_t w) { return (float)(w >> 8) * (1.0f / 16777216.0f); }
// The words a surviving vertex consumes run up to index s + 2 of the two blocks (s: the emitter index's position, below).
APT_HD bool window_spans(uint32_t s) { return s + 2u >= 4u; }
// roulette: the vertex draws it, and dies when the draw exceeds `mx`;  relight: the emitter index is drawn twice;  c[]: the first block
// (generated here unless `have_first`: the camera-fed kernel hands over the words the jitter's pass left, only c[d0 & 3 ..] are read).
// false: the roulette ended the path (one word consumed).
template <typename Any>
APT_HD bool window_open(DrawWindow& w, uint32_t key0, uint32_t key1, uint32_t ctr0, uint32_t d0, bool roulette, float mx, bool relight,
                        uint32_t c[4], bool have_first, Any&& any) {
    const uint32_t b = d0 >> 2, off = d0 & 3u;
    if (!have_first) philox4x32_10(ctr0, b, 0u, 0u, key0, key1, c);
    const uint32_t c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3];
    w.draw = d0; w.rr = 0u;
    bool live = true;
    if (roulette) {
        w.rr = (off & 2u) ? ((off & 1u) ? c3 : c2) : ((off & 1u) ? c1 : c0);
        w.draw = d0 + 1u;
        live = !(window_unit(w.rr) > mx);
    }
    const uint32_t s = off + (roulette ? 1u : 0u) + (relight ? 1u : 0u);      // 0 .. 5
    uint32_t n[4] = {0u, 0u, 0u, 0u};
    if (any(live && window_spans(s))) philox4x32_10(ctr0, b + 1u, 0u, 0u, key0, key1, n);
    // two blocks, eight words W[0 .. 7]; e = W[s], u = W[s + 1], W[s + 2]: a select per bit of s
    const bool hi = (s & 4u) != 0u, b1 = (s & 2u) != 0u, b0 = (s & 1u) != 0u;
    const uint32_t x0 = hi ? n[0] : c0, x1 = hi ? n[1] : c1, x2 = hi ? n[2] : c2, x3 = hi ? n[3] : c3;      // (s >= 4: s & 3 <= 1, nothing past x3 is read)
    const uint32_t y0 = b1 ? x2 : x0, y1 = b1 ? x3 : x1, y2 = b1 ? n[0] : x2, y3 = b1 ? n[1] : x3;
    w.e = b0 ? y1 : y0; w.u[0] = b0 ? y2 : y1; w.u[1] = b0 ? y3 : y2;
    return live;
}
// the draw sites: the emitter index (either draw of it), then the direction's two floats in order
APT_HD int32_t rng_int(DrawWindow& w) { w.draw++; return (int32_t)w.e; }
APT_HD float rng_float(DrawWindow& w) { const uint32_t v = w.u[0]; w.u[0] = w.u[1]; w.draw++; return window_unit(v); }
// Python-style modulo: the reference's `ti.random(int) % n` is non-negative
APT_HD int pymod(int a, int n) { int m = a % n; return (m < 0) ? m + n : m; }
