// tests only, CPU build: the plain-C model of the pair form of Keccak-f[1600] and of the steady-state draws (csrc/keccak.h
// keccak_f1600_pair_model, merlin_rng_fill64_bulk_pair_model: a state as two arrays of 25 words, every partner read explicit), as a
// stand-alone program under AddressSanitizer + UBSan.  The phase functions the model is made of are the ones the device runs.
//
//   keccak_pair_check perm   : reads n x 200 bytes of states from stdin, writes the n permuted states to stdout (tests/
//                              test_keccak_pair_host.py compares them with the Python permutation)
//   keccak_pair_check draws  : 5 draws of the pair model against the one-lane merlin_rng_fill64_bulk and against merlin_rng_fill, from
//                              the state a TranscriptRng is in after its first draw; prints "keccak_pair_check ok"
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../dusk_blindbidproof_amd/csrc/keccak.h"

using namespace bbp;

static int perm() {
    std::vector<uint8_t> in;
    uint8_t buf[4096];
    for (size_t k; (k = fread(buf, 1, sizeof buf, stdin)) > 0;) in.insert(in.end(), buf, buf + k);
    if (in.size() % 200) return 2;
    for (size_t s = 0; s < in.size(); s += 200) {
        u32 lo[25], hi[25];
        for (int i = 0; i < 25; i++) {
            u64 w = 0;
            for (int b = 7; b >= 0; b--) w = (w << 8) | in[s + 8 * i + b];
            lo[i] = (u32)w, hi[i] = (u32)(w >> 32);
        }
        keccak_f1600_pair_model(lo, hi);
        for (int i = 0; i < 25; i++) {
            const u64 w = ((u64)hi[i] << 32) | lo[i];
            for (int b = 0; b < 8; b++) in[s + 8 * i + b] = (uint8_t)(w >> (8 * b));
        }
    }
    return fwrite(in.data(), 1, in.size(), stdout) == in.size() ? 0 : 3;
}

static int draws() {
    const u32 COUNT = 5;
    const uint8_t label[] = {'k', 'e', 'c', 'c', 'a', 'k', '_', 'p', 'a', 'i', 'r'}, wl[] = {'w'};
    uint8_t witness[32], seed[32], first[64];
    for (int i = 0; i < 32; i++) witness[i] = (uint8_t)(7 * i + 1), seed[i] = (uint8_t)(251 - 3 * i);
    merlin_transcript t;
    merlin_init(t, label, sizeof label);
    merlin_rng_rekey(t, wl, sizeof wl, witness, 32);
    merlin_rng_finalize(t, seed);
    merlin_rng_fill(t, first, 64);  // the first draw leaves the sponge in the steady state
    merlin_transcript one = t, pair = t, bytes = t;
    u32 raw_one[COUNT * 16], raw_pair[COUNT * 16];
    memset(raw_one, 0xa5, sizeof raw_one);
    memset(raw_pair, 0x5a, sizeof raw_pair);
    if (!merlin_rng_fill64_bulk(one, COUNT, raw_one) || !merlin_rng_fill64_bulk_pair_model(pair, COUNT, raw_pair)) return 4;
    if (memcmp(raw_one, raw_pair, sizeof raw_one)) return 5;
    if (memcmp(one.st, pair.st, sizeof one.st) || one.pos != pair.pos || one.pos_begin != pair.pos_begin || one.cur_flags != pair.cur_flags) return 6;
    for (u32 c = 0; c < COUNT; c++) {  // ... and both are what the byte-wise transcript draws
        uint8_t b[64];
        merlin_rng_fill(bytes, b, 64);
        for (int i = 0; i < 16; i++) {
            const u32 w = (u32)b[4 * i] | ((u32)b[4 * i + 1] << 8) | ((u32)b[4 * i + 2] << 16) | ((u32)b[4 * i + 3] << 24);
            if (w != raw_pair[16 * c + i]) return 7;
        }
    }
    if (memcmp(bytes.st, pair.st, sizeof pair.st)) return 8;
    // a sponge that is not in the steady state is refused and left alone
    merlin_transcript off = t;
    off.pos = 63;
    const merlin_transcript keep = off;
    if (merlin_rng_fill64_bulk_pair_model(off, 1, raw_pair) || memcmp(&off, &keep, sizeof off)) return 9;
    puts("keccak_pair_check ok");
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "perm")) return perm();
    if (argc == 2 && !strcmp(argv[1], "draws")) return draws();
    fputs("usage: keccak_pair_check perm|draws\n", stderr);
    return 1;
}
