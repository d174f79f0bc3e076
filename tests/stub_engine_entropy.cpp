// TEST INFRASTRUCTURE.  The stub engine of tests/stub_engine.cpp, unchanged, plus bbp_set_entropy_source for the server's --entropy
// flag: every value it is given is appended, one decimal number per line, to the file STUB_ENTROPY_LOG names, and the value in
// STUB_ENTROPY_REJECT (if set) is rejected with BBP_ERR_BAD_ARG, as an engine older than that source would.
#include "stub_engine.cpp"

extern "C" int32_t bbp_set_entropy_source(bbp_ctx*, int32_t source) {
    if (const char* path = getenv("STUB_ENTROPY_LOG")) {
        if (FILE* f = fopen(path, "a")) {
            fprintf(f, "%d\n", (int)source);
            fclose(f);
        }
    }
    const char* rej = getenv("STUB_ENTROPY_REJECT");
    if (rej && atoi(rej) == source) {
        t_err = "stub: unknown entropy source";
        return BBP_ERR_BAD_ARG;
    }
    return BBP_OK;
}
