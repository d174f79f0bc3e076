// TEST INFRASTRUCTURE.  The stub engine of tests/stub_engine.cpp, unchanged, behind one more switch that the pipelining tests need:
// STUB_REFUSE_ITEMS=n makes bbp_prove_async refuse a bid list of exactly n entries AT ONCE (BBP_ERR_BAD_ARG, the callback never
// fires) -- the "engine refuses a prove at once" outcome, which no request that passes the server's own parse can get from the
// plain stub.  Without the variable it is the plain stub, so the sanitizer builds of the stub use this file too.
#define bbp_prove_async stub_prove_async_plain
#include "stub_engine.cpp"
#undef bbp_prove_async

extern "C" int32_t bbp_prove_async(bbp_ctx* c, const uint8_t s7[7 * 32], const uint8_t* pub, uint32_t N, uint64_t toggle, const uint8_t* ent, uint8_t* out,
                                   bbp_done_fn done, void* user) {
    static const uint32_t refuse = getenv("STUB_REFUSE_ITEMS") ? (uint32_t)atoi(getenv("STUB_REFUSE_ITEMS")) : 0;
    if (refuse && N == refuse) {
        t_err = "stub: refused at once";
        return BBP_ERR_BAD_ARG;
    }
    return stub_prove_async_plain(c, s7, pub, N, toggle, ent, out, done, user);
}
