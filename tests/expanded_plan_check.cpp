// Host program of tests/test_expanded_draw_host.py: csrc/prove_plan.h with the blinding-draw setting, driven from standard input, one plan
// per line of output.  Stand-alone (its own main), built with -fsanitize=address,undefined and run as it is.
//   plan DRAW B INFLIGHT BUSY DEEP_MODE LAST_SLICED CALLS N1 HWQ [NAME TEXT]...
// DRAW: ProveKnobs::blinding_draw (0 MERLIN, 1 EXPANDED); the state a context would carry; knobs by environment name over the defaults.
// Prints: call deep behind_sliced dual open_stream par coop chain prefix_form serial_blk cblk rotate heavy_stream slices open_on_chain
//         chain_stream roles raw_index raw_bytes(B, N1) bound0..bound<slices> | trace_line
#include <stdio.h>
#include <string.h>

#include "../dusk_blindbidproof_amd/csrc/prove_plan.h"

using namespace bbp;

int main() {
    char line[1024];
    while (fgets(line, sizeof line, stdin)) {
        char* save = nullptr;
        const char* cmd = strtok_r(line, " \n", &save);
        if (!cmd) continue;
        if (strcmp(cmd, "plan")) return 5;
        long v[9];
        for (long& x : v) {
            const char* tok = strtok_r(nullptr, " \n", &save);
            if (!tok) return 2;
            x = strtol(tok, nullptr, 10);
        }
        ProveKnobs k;
        ProveRuleState st;
        k.blinding_draw = (int)v[0];
        k.hw_queues = (int)v[8];
        st.deep_mode = v[4] != 0, st.last_sliced = v[5] != 0, st.calls = (uint32_t)v[6];
        while (const char* name = strtok_r(nullptr, " \n", &save)) {
            const char* text = strtok_r(nullptr, " \n", &save);
            if (!text || !k.set(name, text)) return 4;
        }
        const uint32_t B = (uint32_t)v[1];
        const bool busy = v[3] != 0;
        const ProvePlan p = plan_prove(k, st, B, (int)v[2], [&] { return busy; });
        printf("%u %d %d %d %d %d %d %d %u %u %u %d %d %u %d %d %u %d %zu", p.call, (int)p.deep, (int)p.behind_sliced, (int)p.dual, p.open_stream, p.par, (int)p.coop,
               (int)p.chain, p.prefix_form, p.serial_blk, p.cblk, (int)p.rotate, p.heavy_stream, p.slices, (int)p.open_on_chain, p.chain_stream, p.roles(),
               p.raw_index(), p.raw_bytes(B, (uint32_t)v[7]));
        for (uint32_t i = 0; p.slices && i <= p.slices; i++) printf(" %u", p.slice_first(B, i));
        printf(" | %s", p.trace_line(p.call, B, (int)v[2]).c_str());
    }
    return 0;
}
