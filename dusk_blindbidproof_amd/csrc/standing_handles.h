// Which of a handle's BBP_STANDING_MAX_OPEN standings are open (include/bbp.h "Standing of a round").  A new standing takes the lowest
// free handle, so a closed handle is handed out again.  Plain C++, no HIP: context.h holds one, tests/round_standing_check.cpp runs it.
#pragma once
#include <stdint.h>

#include "../../include/bbp.h"

namespace bbp {

struct StandingHandles {
    bool used[BBP_STANDING_MAX_OPEN] = {};
    // the new standing's handle, or BBP_STANDING_MAX_OPEN when every one is open
    uint32_t take() {
        uint32_t h = 0;
        while (h < BBP_STANDING_MAX_OPEN && used[h]) h++;
        if (h < BBP_STANDING_MAX_OPEN) used[h] = true;
        return h;
    }
    bool is_open(uint32_t h) const { return h < BBP_STANDING_MAX_OPEN && used[h]; }
    // false: no open standing has this handle
    bool release(uint32_t h) {
        if (!is_open(h)) return false;
        used[h] = false;
        return true;
    }
};

}  // namespace bbp
