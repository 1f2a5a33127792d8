"""The draw window (csrc/rng.hpp DrawWindow) against the generator it stands in for, on the CPU.

A traced-kernel vertex without area lights draws [roulette] emitter index [emitter index again] u1 u2.  window_open fills a DrawWindow
with exactly those words; the stream is the oracle's by definition, so for every entry draw index 0 .. 63, with and without a roulette
draw, with a roulette that ends the path, with and without the second index draw, and for a first block handed over instead of
generated, the host program below checks that
  - the window's words are those of successive rng_u32 calls on the same key and counter,
  - the draw index afterwards is the same,
  - the second block is asked for exactly when a consumed word lies in it.
rng.hpp is compiled for the host by hipcc (no GPU is touched: the program makes no HIP call)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

PROGRAM = r"""
#include <hip/hip_runtime.h>
#include <cstdio>
#include "%(root)s/adapt_amd/csrc/rng.hpp"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { printf("FAIL %%s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// mode 0: no roulette; 1: the roulette is drawn and survived; 2: the roulette ends the path
static void one(uint32_t key0, uint32_t key1, uint32_t ctr0, uint32_t d0, int mode, bool relight, bool have_first) {
    Philox r; rng_init(r, key0, key1, ctr0, d0);
    uint32_t want_rr = 0, want_e = 0, want_u[2] = {0, 0}, consumed = 0;
    if (mode != 0) { want_rr = rng_u32(r); consumed++; }
    if (mode != 2) {
        want_e = rng_u32(r); consumed++;
        if (relight) { want_e = rng_u32(r); consumed++; }
        want_u[0] = rng_u32(r); want_u[1] = rng_u32(r); consumed += 2;
    }
    const bool want_second = ((d0 & 3u) + consumed - 1u) >= 4u;

    uint32_t c[4] = {0xdeadbeefu, 0xdeadbeefu, 0xdeadbeefu, 0xdeadbeefu};
    if (have_first) {                                    // the block of d0, of which only the words from d0 & 3 on may be read
        uint32_t blk[4]; philox4x32_10(ctr0, d0 >> 2, 0u, 0u, key0, key1, blk);
        for (uint32_t k = d0 & 3u; k < 4u; k++) c[k] = blk[k];
    }
    DrawWindow w; rng_init(w, key0, key1, ctr0, d0);
    int votes = 0; bool second = false;
    // the roulette compares its float with mx: 2 is never exceeded, -1 always
    const bool live = window_open(w, key0, key1, ctr0, d0, mode != 0, mode == 2 ? -1.0f : 2.0f, relight, c, have_first,
                                  [&](bool v) { votes++; second = v; return v; });
    CHECK(votes == 1, "d0 %%u mode %%d: %%d votes", d0, mode, votes);
    CHECK(live == (mode != 2), "d0 %%u mode %%d relight %%d", d0, mode, (int)relight);
    CHECK(second == want_second, "d0 %%u mode %%d relight %%d first %%d: second block %%d, consumed words reach it: %%d", d0, mode, (int)relight, (int)have_first, (int)second, (int)want_second);
    if (mode != 0) CHECK(w.rr == want_rr, "d0 %%u mode %%d: roulette word %%08x, stream %%08x", d0, mode, w.rr, want_rr);
    if (live) {
        const uint32_t e1 = (uint32_t)rng_int(w);
        const uint32_t e = relight ? (uint32_t)rng_int(w) : e1;
        CHECK(e == want_e && e1 == want_e, "d0 %%u mode %%d relight %%d: index %%08x, stream %%08x", d0, mode, (int)relight, e, want_e);
        const float u0 = rng_float(w), u1 = rng_float(w);
        CHECK(u0 == window_unit(want_u[0]) && u1 == window_unit(want_u[1]), "d0 %%u mode %%d relight %%d first %%d: floats %%a %%a, stream %%a %%a", d0, mode, (int)relight, (int)have_first, u0, u1, window_unit(want_u[0]), window_unit(want_u[1]));
    }
    CHECK(w.draw == r.draw, "d0 %%u mode %%d relight %%d: draw index %%u, stream %%u", d0, mode, (int)relight, w.draw, r.draw);
}

int main() {
    // the float of a word is what rng_float makes of it
    { Philox r; rng_init(r, 7u, 9u, 3u, 5u); Philox q = r; const uint32_t wd = rng_u32(q); CHECK(rng_float(r) == window_unit(wd), "window_unit"); }
    int cases = 0;
    const uint32_t keys[3][3] = {{0u, 0u, 1u}, {123456u, 42u, 17u}, {0xffffffffu, 0x9e3779b9u, 1025u}};
    for (int k = 0; k < 3; k++)
        for (uint32_t d0 = 0; d0 < 64u; d0++)
            for (int mode = 0; mode < 3; mode++)
                for (int relight = 0; relight < 2; relight++)
                    for (int first = 0; first < 2; first++) { one(keys[k][0], keys[k][1], keys[k][2], d0, mode, relight != 0, first != 0); cases++; }
    printf("%%d cases, %%d failures\n", cases, failures);
    return failures ? 1 : 0;
}
"""


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_draw_window_serves_the_stream_of_rng_u32(tmp_path):
    src = tmp_path / "window_host.hip"
    src.write_text(PROGRAM % {"root": ROOT})
    exe = tmp_path / "window_host"
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-fno-fast-math", "-ffp-contract=off", str(src), "-o", str(exe)],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(run.stdout[-3000:])
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-1000:]
    assert "2304 cases, 0 failures" in run.stdout
