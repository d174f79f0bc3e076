// Host program of tests/test_prove_chain_plan_host.py: csrc/prove_plan.h driven from standard input, one plan per line of output.
// Stand-alone (its own main) so that it can be built with -fsanitize=address,undefined and run as it is.
//   reset HWQ KNOB [NAME TEXT]...   a fresh context: hw_queues, BBP_OPEN_ON_CHAIN (-1 = unset), further knobs by environment name
//   call B INFLIGHT BUSY            plan_prove on that context's state; then last_sliced = !rotate, as the driver sets it
// A call prints: call deep behind_sliced dual open_stream par coop chain prefix_form serial_blk cblk rotate heavy_stream slices
//                | open_on_chain chain_stream roles raw_index | trace_line
#include <stdio.h>
#include <string.h>

#include "../dusk_blindbidproof_amd/csrc/prove_plan.h"

using namespace bbp;

int main() {
    ProveKnobs k;
    ProveRuleState st;
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        char* save = nullptr;
        const char* cmd = strtok_r(line, " \n", &save);
        if (!cmd) continue;
        if (!strcmp(cmd, "reset")) {
            k = ProveKnobs();
            st = ProveRuleState();
            const char* hwq = strtok_r(nullptr, " \n", &save);
            const char* knob = strtok_r(nullptr, " \n", &save);
            if (!hwq || !knob) return 2;
            k.hw_queues = atoi(hwq);
            if (atoi(knob) >= 0 && !k.set("BBP_OPEN_ON_CHAIN", knob)) return 3;
            while (const char* name = strtok_r(nullptr, " \n", &save)) {
                const char* text = strtok_r(nullptr, " \n", &save);
                if (!text || !k.set(name, text)) return 4;
            }
        } else if (!strcmp(cmd, "call")) {
            const char* b = strtok_r(nullptr, " \n", &save);
            const char* inflight = strtok_r(nullptr, " \n", &save);
            const char* busy = strtok_r(nullptr, " \n", &save);
            if (!b || !inflight || !busy) return 2;
            const bool is_busy = atoi(busy) != 0;
            const ProvePlan p = plan_prove(k, st, (uint32_t)strtoul(b, nullptr, 10), atoi(inflight), [&] { return is_busy; });
            st.last_sliced = !p.rotate;
            printf("%u %d %d %d %d %d %d %d %u %u %u %d %d %u | %d %d %u %d | %s", p.call, (int)p.deep, (int)p.behind_sliced, (int)p.dual, p.open_stream, p.par,
                   (int)p.coop, (int)p.chain, p.prefix_form, p.serial_blk, p.cblk, (int)p.rotate, p.heavy_stream, p.slices, (int)p.open_on_chain, p.chain_stream,
                   p.roles(), p.raw_index(), p.trace_line(p.call, (uint32_t)strtoul(b, nullptr, 10), atoi(inflight)).c_str());
        } else {
            return 5;
        }
    }
    return 0;
}
