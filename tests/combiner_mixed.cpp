// TEST INFRASTRUCTURE: the call combiner's merged verify class (dusk_blindbidproof_amd/csrc/submit.cpp, the product's own code) behind
// a stand-in engine that records every batch it is handed.  With a mixed-N runner installed (Combiner::set_mixed_verify) and mixing on,
// verify requests of any list length and record layout leave as ONE batch: uniform batches still go to verify_batch_locked, any other
// is packed row by row in queue order and goes to the runner.  Without a runner, or with mixing off, batches are one class each.
// Prove requests are one class per batch whatever the switch says.
//   combiner_mixed          the scenarios below, one after the other, then the many-thread run
//   combiner_mixed stress   the many-thread run alone
// The same source is built plain and with -fsanitize=thread.  Prints one line per scenario; exit code 0 = all of them passed.
#include <stdio.h>
#include <string.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../dusk_blindbidproof_amd/csrc/submit.h"

struct Call {
    int what;  // 0 prove_batch_locked, 1 verify_batch_locked, 2 the mixed runner
    uint32_t B, N, ver;
    std::vector<uint32_t> ns;
    std::vector<uint8_t> vers, bytes;
};
struct bbp_ctx {
    std::mutex m;
    std::vector<Call> calls;
    std::atomic<int> bad{0};  // a batch that broke a rule the stand-in can see (a row of another class in a uniform call, max_batch)
    uint32_t max_batch = 4096;
    bool fail_mixed = false;
    bool keep_bytes = true;
};

static size_t vrow_len(uint32_t N, uint32_t ver) { return (ver ? 1217u : 1121u) + 32 * (4 + (size_t)N) + 96 + 32 * (size_t)N; }
static size_t prow_len(uint32_t N) { return 7 * 32 + 32 * (size_t)N + 8; }
// a row says what it is: byte 0 the layout (as a real record does), byte 1 a tag, byte 2 its list length; the stand-in's "verdict"
// is a function of the row's own bytes
static int32_t verdict(const uint8_t* row) { return (int32_t)((row[1] * 7u + row[2] + row[0]) % 5u); }

namespace bbp {
int32_t prove_batch_locked(bbp_ctx* c, uint32_t B, uint32_t N, const uint8_t* in, const uint8_t*, uint8_t* out, int32_t* status, std::string*) {
    const size_t rec = 1121 + 32 * (4 + (size_t)N);
    if (B == 0 || B > c->max_batch) c->bad++;
    for (uint32_t i = 0; i < B; i++) {
        const uint8_t* row = in + prow_len(N) * i;
        if (row[2] != (uint8_t)N) c->bad++;  // one list length per prove batch
        status[i] = 0;
        memset(out + rec * i, row[1], rec);
    }
    std::lock_guard<std::mutex> lk(c->m);
    c->calls.push_back(Call{0, B, N, 0, {}, {}, {}});
    return 0;
}
int32_t verify_batch_locked(bbp_ctx* c, uint32_t B, uint32_t N, uint32_t ver, const uint8_t* in, int32_t* status, std::string*) {
    if (B == 0 || B > c->max_batch) c->bad++;
    for (uint32_t i = 0; i < B; i++) {
        const uint8_t* row = in + vrow_len(N, ver) * i;
        if (row[2] != (uint8_t)N || row[0] != (uint8_t)ver) c->bad++;  // a uniform call holds one list length and one layout
        status[i] = verdict(row);
    }
    usleep(200);
    std::lock_guard<std::mutex> lk(c->m);
    c->calls.push_back(Call{1, B, N, ver, {}, {}, {}});
    return 0;
}
}  // namespace bbp

static int32_t mixed_runner(bbp_ctx* c, uint32_t B, const uint32_t* Ns, const uint8_t* vers, const uint8_t* in, int32_t* status, std::string* err) {
    if (B == 0 || B > c->max_batch) c->bad++;
    Call k{2, B, 0, 0, std::vector<uint32_t>(Ns, Ns + B), std::vector<uint8_t>(vers, vers + B), {}};
    size_t off = 0;
    bool differ = false;
    for (uint32_t i = 0; i < B; i++) {
        const uint8_t* row = in + off;
        if (row[2] != (uint8_t)Ns[i] || row[0] != vers[i]) c->bad++;  // Ns / vers describe the rows as packed
        if (Ns[i] != Ns[0] || vers[i] != vers[0]) differ = true;
        status[i] = verdict(row);
        off += vrow_len(Ns[i], vers[i]);
    }
    if (!differ) c->bad++;  // a batch of one list length and layout belongs to verify_batch_locked
    if (c->keep_bytes) k.bytes.assign(in, in + off);
    usleep(200);
    {
        std::lock_guard<std::mutex> lk(c->m);
        c->calls.push_back(std::move(k));
    }
    if (c->fail_mixed) {
        *err = "stand-in: the mixed call failed";
        return 5;
    }
    return 0;
}

// ---- requests ------------------------------------------------------------------------------------------------------------------
struct Sink {  // where the completion hooks of a scenario report
    std::mutex m;
    std::condition_variable cv;
    int done = 0, wrong = 0;
    std::vector<std::pair<int32_t, std::string>> results;  // by request index
};
struct Tagged {
    bbp::Request r;
    Sink* sink = nullptr;
    int index = 0;
    int32_t want = 0;
};
static void hook(bbp::Request* r) {
    Tagged* t = reinterpret_cast<Tagged*>(r->user);
    Sink* s = t->sink;
    std::lock_guard<std::mutex> lk(s->m);
    if ((size_t)t->index >= s->results.size()) s->results.resize(t->index + 1);
    s->results[t->index] = {r->status, r->err};
    if (r->status != t->want) s->wrong++;
    s->done++;
    s->cv.notify_all();
}
static thread_local uint32_t g_seed = 12345;  // filler bytes of the rows
static uint8_t rnd() {
    g_seed = g_seed * 1664525u + 1013904223u;
    return (uint8_t)(g_seed >> 24);
}
static Tagged* make_verify(Sink* s, int index, uint32_t N, uint32_t ver, uint8_t tag) {
    Tagged* t = new Tagged();
    t->sink = s;
    t->index = index;
    t->r.own_in.resize(vrow_len(N, ver));
    for (auto& b : t->r.own_in) b = rnd();
    t->r.own_in[0] = (uint8_t)ver;
    t->r.own_in[1] = tag;
    t->r.own_in[2] = (uint8_t)N;
    t->r.kind = 1;
    t->r.N = N;
    t->r.rec_ver = ver;
    t->r.in = t->r.own_in.data();
    t->r.in_len = t->r.own_in.size();
    t->r.on_done = hook;
    t->r.user = t;
    t->want = verdict(t->r.in);
    return t;
}
static Tagged* make_prove(Sink* s, int index, uint32_t N, uint8_t tag) {
    Tagged* t = new Tagged();
    t->sink = s;
    t->index = index;
    t->r.own_in.assign(prow_len(N), 0);
    t->r.own_in[1] = tag;
    t->r.own_in[2] = (uint8_t)N;
    t->r.kind = 0;
    t->r.N = N;
    t->r.in = t->r.own_in.data();
    t->r.in_len = t->r.own_in.size();
    t->r.out = new uint8_t[1121 + 32 * (4 + N)];
    t->r.on_done = hook;
    t->r.user = t;
    t->want = 0;
    return t;
}
static void wait_done(Sink& s, int n) {
    std::unique_lock<std::mutex> lk(s.m);
    s.cv.wait(lk, [&] { return s.done >= n; });
}
static void drop(std::vector<Tagged*>& v) {
    for (Tagged* t : v) {
        delete[] t->r.out;
        delete t;
    }
    v.clear();
}

static int g_failed = 0;
static void report(const char* name, bool ok, const std::string& why = "") {
    printf("%s %s%s%s\n", ok ? "PASS" : "FAIL", name, why.empty() ? "" : ": ", why.c_str());
    fflush(stdout);
    if (!ok) g_failed++;
}
static const uint32_t WINDOW_US = 150000;  // long enough that a burst submitted from one thread lands in one window

struct Spec {
    uint32_t N, ver;
};
// the burst of the mixed scenarios: three list lengths, both layouts
static const Spec BURST[] = {{3, 0}, {1, 0}, {7, 1}, {3, 1}, {1, 0}, {7, 0}, {3, 0}, {7, 1}, {1, 1}, {3, 0}, {7, 0}, {1, 0}};
static const int NB = sizeof BURST / sizeof BURST[0];

static void submit_burst(bbp::Combiner& comb, bbp_ctx& ctx, Sink& sink, std::vector<Tagged*>& reqs) {
    for (int i = 0; i < NB; i++) reqs.push_back(make_verify(&sink, i, BURST[i].N, BURST[i].ver, (uint8_t)(3 * i + 1)));
    for (Tagged* t : reqs)
        if (!comb.submit_async(&ctx, &t->r)) sink.wrong++;
    wait_done(sink, NB);
}

// 1. three list lengths and both layouts arrive together, runner installed: ONE mixed batch, rows / Ns / vers in queue order, own statuses
static void one_mixed_batch() {
    bbp_ctx ctx;
    Sink sink;
    std::vector<Tagged*> reqs;
    std::string why;
    {
        bbp::Combiner comb;
        comb.set_mixed_verify(mixed_runner);
        comb.configure(WINDOW_US, 4096);
        if (!comb.verify_mixing()) why += " verify_mixing() is false with a runner installed;";
        submit_burst(comb, ctx, sink, reqs);
        uint64_t calls = 0, nreq = 0;
        comb.stats(&calls, &nreq, nullptr);
        if (calls != 1 || nreq != (uint64_t)NB) why += " stats: " + std::to_string(calls) + " calls;";
    }
    if (ctx.calls.size() != 1 || ctx.calls[0].what != 2 || ctx.calls[0].B != (uint32_t)NB)
        why += " expected one mixed call of " + std::to_string(NB) + ", got " + std::to_string(ctx.calls.size()) + " call(s);";
    else {
        std::vector<uint8_t> want;
        for (int i = 0; i < NB; i++) {
            if (ctx.calls[0].ns[i] != BURST[i].N || ctx.calls[0].vers[i] != BURST[i].ver) why += " Ns / vers differ at row " + std::to_string(i) + ";";
            want.insert(want.end(), reqs[i]->r.own_in.begin(), reqs[i]->r.own_in.end());
        }
        if (want != ctx.calls[0].bytes) why += " packed bytes are not the requests in queue order;";
    }
    bool varied = false;
    for (int i = 0; i < NB; i++) {
        if (sink.results[i].first != reqs[i]->want) why += " request " + std::to_string(i) + " got another row's status;";
        if (reqs[i]->want != reqs[0]->want) varied = true;
    }
    if (!varied) why += " (the scenario's statuses are all equal: it shows nothing);";
    if (ctx.bad) why += " stand-in saw an inconsistent batch;";
    report("one_mixed_batch", why.empty(), why);
    drop(reqs);
}

// 2. one list length, one layout: verify_batch_locked as ever, the runner is not called
static void uniform_goes_uniform() {
    bbp_ctx ctx;
    Sink sink;
    std::vector<Tagged*> reqs;
    {
        bbp::Combiner comb;
        comb.set_mixed_verify(mixed_runner);
        comb.configure(WINDOW_US, 4096);
        for (int i = 0; i < 8; i++) reqs.push_back(make_verify(&sink, i, 5, 0, (uint8_t)(i + 1)));
        for (Tagged* t : reqs)
            if (!comb.submit_async(&ctx, &t->r)) sink.wrong++;
        wait_done(sink, 8);
    }
    const bool ok = ctx.calls.size() == 1 && ctx.calls[0].what == 1 && ctx.calls[0].B == 8 && ctx.calls[0].N == 5 && !sink.wrong && !ctx.bad;
    report("uniform_goes_uniform", ok, ok ? "" : std::to_string(ctx.calls.size()) + " call(s), first of kind " + std::to_string(ctx.calls.empty() ? -1 : ctx.calls[0].what));
    drop(reqs);
}

// 3. prove requests of three list lengths: one class per batch, runner or not
static void prove_stays_per_class() {
    bbp_ctx ctx;
    Sink sink;
    std::vector<Tagged*> reqs;
    {
        bbp::Combiner comb;
        comb.set_mixed_verify(mixed_runner);
        comb.configure(WINDOW_US, 4096);
        const uint32_t ns[3] = {2, 4, 9};
        for (int i = 0; i < 9; i++) reqs.push_back(make_prove(&sink, i, ns[i % 3], (uint8_t)(i + 1)));
        for (Tagged* t : reqs)
            if (!comb.submit_async(&ctx, &t->r)) sink.wrong++;
        wait_done(sink, 9);
    }
    bool ok = ctx.calls.size() == 3 && !sink.wrong && !ctx.bad;
    for (const Call& c : ctx.calls) ok = ok && c.what == 0 && c.B == 3;
    for (int i = 0; i < 9 && ok; i++) ok = reqs[i]->r.out[0] == (uint8_t)(i + 1);
    report("prove_stays_per_class", ok, ok ? "" : std::to_string(ctx.calls.size()) + " prove call(s), " + std::to_string(ctx.bad.load()) + " inconsistent");
    drop(reqs);
}

// 4. no runner / mixing off: the burst leaves per class, as before
static void per_class(bool with_runner) {
    bbp_ctx ctx;
    Sink sink;
    std::vector<Tagged*> reqs;
    std::string why;
    {
        bbp::Combiner comb;
        if (with_runner) {
            comb.set_mixed_verify(mixed_runner);
            comb.set_verify_mixing(false);
        }
        if (comb.verify_mixing()) why += " verify_mixing() is true;";
        comb.configure(WINDOW_US, 4096);
        submit_burst(comb, ctx, sink, reqs);
    }
    if (ctx.calls.size() != 6) why += " expected 6 calls (three list lengths, two layouts), got " + std::to_string(ctx.calls.size()) + ";";
    for (const Call& c : ctx.calls)
        if (c.what != 1) why += " a call of kind " + std::to_string(c.what) + ";";
    if (sink.wrong) why += " wrong statuses;";
    if (ctx.bad) why += " a batch held two classes;";
    report(with_runner ? "mixing_off_is_per_class" : "no_runner_is_per_class", why.empty(), why);
    drop(reqs);
}

// 5. the mixed call fails: every member gets the call's status and message
static void failing_mixed_call() {
    bbp_ctx ctx;
    ctx.fail_mixed = true;
    Sink sink;
    std::vector<Tagged*> reqs;
    {
        bbp::Combiner comb;
        comb.set_mixed_verify(mixed_runner);
        comb.configure(WINDOW_US, 4096);
        for (int i = 0; i < NB; i++) {
            reqs.push_back(make_verify(&sink, i, BURST[i].N, BURST[i].ver, (uint8_t)(3 * i + 1)));
            reqs.back()->want = 5;
        }
        for (Tagged* t : reqs)
            if (!comb.submit_async(&ctx, &t->r)) sink.wrong++;
        wait_done(sink, NB);
    }
    bool ok = ctx.calls.size() == 1 && ctx.calls[0].what == 2 && !sink.wrong;
    for (int i = 0; i < NB && ok; i++) ok = sink.results[i].first == 5 && sink.results[i].second == "stand-in: the mixed call failed";
    report("failing_mixed_call", ok);
    drop(reqs);
}

// 6. blocking and asynchronous requests of different list lengths in one batch
static void blocking_and_async() {
    bbp_ctx ctx;
    Sink sink;
    std::vector<Tagged*> reqs;
    std::atomic<int> wrong_blocking{0};
    {
        bbp::Combiner comb;
        comb.set_mixed_verify(mixed_runner);
        comb.configure(2 * WINDOW_US, 4096);
        for (int i = 0; i < 6; i++) reqs.push_back(make_verify(&sink, i, 2 + i, i & 1, (uint8_t)(5 * i + 2)));
        for (Tagged* t : reqs)
            if (!comb.submit_async(&ctx, &t->r)) sink.wrong++;
        std::vector<std::thread> th;
        for (int i = 0; i < 6; i++)
            th.emplace_back([&, i] {
                Tagged* t = make_verify(nullptr, 0, 20 + i, (i >> 1) & 1, (uint8_t)(11 * i + 3));
                if (comb.submit(&ctx, t->r) != t->want) wrong_blocking++;
                delete t;
            });
        for (auto& t : th) t.join();
        wait_done(sink, 6);
    }
    size_t rows = 0;
    for (const Call& c : ctx.calls) rows += c.B;
    const bool ok = rows == 12 && ctx.calls.size() == 1 && ctx.calls[0].what == 2 && !sink.wrong && !wrong_blocking && !ctx.bad;
    report("blocking_and_async", ok, ok ? "" : std::to_string(ctx.calls.size()) + " call(s), " + std::to_string(rows) + " rows, wrong " + std::to_string(sink.wrong + wrong_blocking));
    drop(reqs);
}

// 7. many threads, prove and verify, blocking and asynchronous, a short window, small batches; one engine and a pool of three
static void stress(int n_targets, bool mixing) {
    std::vector<bbp_ctx> ctxs(n_targets);
    for (auto& c : ctxs) {
        c.max_batch = 8;
        c.keep_bytes = false;
    }
    const int T = 32, PER = 30;
    std::atomic<int> wrong{0};
    Sink sink;
    std::vector<std::vector<Tagged*>> mine(T);
    {
        bbp::Combiner comb;
        comb.set_mixed_verify(mixed_runner);
        comb.set_verify_mixing(mixing);
        comb.configure(100, 8);
        comb.set_stagger(500);
        if (n_targets > 1) {
            std::vector<bbp_ctx*> t;
            for (auto& c : ctxs) t.push_back(&c);
            comb.set_targets(t);
        }
        std::vector<std::thread> th;
        for (int k = 0; k < T; k++)
            th.emplace_back([&, k] {
                uint32_t s = 977u * (uint32_t)k + 5;
                auto next = [&] { return (s = s * 1103515245u + 12345u) >> 16; };
                for (int j = 0; j < PER; j++) {
                    const uint32_t N = 1 + next() % 3 * 4, ver = next() & 1;
                    const int how = next() % 4;  // 0: blocking verify, 1: asynchronous verify, 2: blocking prove, 3: blocking verify, now and then flipping the switch
                    if (how == 2) {
                        Tagged* t = make_prove(nullptr, 0, N, (uint8_t)next());
                        if (comb.submit(&ctxs[0], t->r) != 0 || t->r.out[0] != t->r.own_in[1]) wrong++;
                        delete[] t->r.out;
                        delete t;
                        continue;
                    }
                    Tagged* t = make_verify(&sink, 0, N, ver, (uint8_t)next());
                    if (how == 1) {
                        t->index = k * PER + j;
                        mine[k].push_back(t);
                        if (!comb.submit_async(&ctxs[0], &t->r)) wrong++;
                    } else {
                        if (how == 3 && (j % 10) == 0) {  // the switch races with batch formation
                            comb.set_verify_mixing(false);
                            comb.set_verify_mixing(mixing);
                        }
                        if (comb.submit(&ctxs[0], t->r) != t->want) wrong++;
                        delete t;
                    }
                }
            });
        for (auto& t : th) t.join();
        int n_async = 0;
        for (auto& v : mine) n_async += (int)v.size();
        wait_done(sink, n_async);
    }
    int bad = 0, mixed_calls = 0;
    for (auto& c : ctxs) {
        bad += c.bad;
        for (const Call& k : c.calls) mixed_calls += k.what == 2;
    }
    for (auto& v : mine) drop(v);
    const bool ok = !wrong && !sink.wrong && !bad && (mixing ? mixed_calls > 0 : mixed_calls == 0);
    char name[64];
    snprintf(name, sizeof name, "stress_%d_target%s_mixing_%s", n_targets, n_targets > 1 ? "s" : "", mixing ? "on" : "off");
    report(name, ok, ok ? "" : "wrong " + std::to_string(wrong + sink.wrong) + ", bad batches " + std::to_string(bad) + ", mixed calls " + std::to_string(mixed_calls));
}

int main(int argc, char** argv) {
    const bool only_stress = argc > 1 && strcmp(argv[1], "stress") == 0;
    if (!only_stress) {
        one_mixed_batch();
        uniform_goes_uniform();
        prove_stays_per_class();
        per_class(false);
        per_class(true);
        failing_mixed_call();
        blocking_and_async();
    }
    stress(1, true);
    stress(3, true);
    stress(1, false);
    printf("RESULT failed %d\n", g_failed);
    return g_failed ? 1 : 0;
}
