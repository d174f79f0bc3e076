// TEST INFRASTRUCTURE: the call combiner's round sharing (dusk_blindbidproof_amd/csrc/submit.cpp, the product's own code) behind a
// stand-in engine that records every call it is handed.  With a rounds runner installed (Combiner::set_round_verify) and sharing on
// (Combiner::set_round_sharing, default off), a verify batch of compact records that holds fewer distinct rounds than requests leaves
// as ONE rounds call: the table is seed || pub_list of every distinct round, numbered by first appearance in queue order, the rows are
// record || score || z_img in queue order.  Bytes decide what a round is, never the hash.  Every other batch takes the path it takes
// with sharing off.
//   combiner_rounds          the scenarios below, one after the other, then the many-thread run
//   combiner_rounds stress   the many-thread run alone
// The same source is built plain and with -fsanitize=thread.  Prints one line per scenario; exit code 0 = all of them passed.
#include <stdio.h>
#include <string.h>
#include <unistd.h>

#include <atomic>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../dusk_blindbidproof_amd/csrc/submit.h"

struct Call {
    int what = 0;  // 1 verify_batch_locked, 2 the mixed runner, 3 the rounds runner
    uint32_t B = 0, N = 0, ver = 0, R = 0;
    std::vector<uint32_t> ns, round_of;  // mixed: Ns; rounds: round_Ns
    std::vector<uint8_t> vers, bytes, table;
    bool operator==(const Call& o) const {
        return what == o.what && B == o.B && N == o.N && ver == o.ver && R == o.R && ns == o.ns && round_of == o.round_of && vers == o.vers &&
               bytes == o.bytes && table == o.table;
    }
};
struct bbp_ctx {
    std::mutex m;
    std::vector<Call> calls;
    std::atomic<int> bad{0};  // a call that broke a rule the stand-in can see
    uint32_t max_batch = 4096;
    bool fail_rounds = false;
    bool keep_bytes = true;
};

static size_t rec_len(uint32_t N, uint32_t ver) { return (ver ? 1217u : 1121u) + 32 * (4 + (size_t)N); }
static size_t vrow_len(uint32_t N, uint32_t ver) { return rec_len(N, ver) + 96 + 32 * (size_t)N; }
static size_t short_len(uint32_t N) { return rec_len(N, 0) + 64; }  // record || score || z_img
static size_t round_len(uint32_t N) { return 32 * (1 + (size_t)N); }
// A row says what it is: byte 0 the layout (as a real record does), byte 1 a tag, byte 2 its list length.  The stand-in's "verdict"
// is a function of the row's own bytes AND of the round it is checked against (first and last byte of seed || pub_list): a row
// that met another request's round gets another verdict.
static int32_t verdict(const uint8_t* row, const uint8_t* round, uint32_t N) {
    return (int32_t)((row[1] * 7u + row[2] + row[0] + round[0] * 3u + round[round_len(N) - 1] * 5u) % 5u);
}

namespace bbp {
int32_t prove_batch_locked(bbp_ctx* c, uint32_t, uint32_t, const uint8_t*, const uint8_t*, uint8_t*, int32_t*, std::string*) {
    c->bad++;  // no scenario proves
    return 6;
}
int32_t verify_batch_locked(bbp_ctx* c, uint32_t B, uint32_t N, uint32_t ver, const uint8_t* in, int32_t* status, std::string*) {
    if (B == 0 || B > c->max_batch) c->bad++;
    Call k;
    k.what = 1, k.B = B, k.N = N, k.ver = ver;
    for (uint32_t i = 0; i < B; i++) {
        const uint8_t* row = in + vrow_len(N, ver) * i;
        if (row[2] != (uint8_t)N || row[0] != (uint8_t)ver) c->bad++;
        status[i] = verdict(row, row + vrow_len(N, ver) - round_len(N), N);
    }
    if (c->keep_bytes) k.bytes.assign(in, in + vrow_len(N, ver) * B);
    usleep(200);
    std::lock_guard<std::mutex> lk(c->m);
    c->calls.push_back(std::move(k));
    return 0;
}
}  // namespace bbp

static int32_t mixed_runner(bbp_ctx* c, uint32_t B, const uint32_t* Ns, const uint8_t* vers, const uint8_t* in, int32_t* status, std::string*) {
    if (B == 0 || B > c->max_batch) c->bad++;
    Call k;
    k.what = 2, k.B = B, k.ns.assign(Ns, Ns + B), k.vers.assign(vers, vers + B);
    size_t off = 0;
    for (uint32_t i = 0; i < B; i++) {
        const uint8_t* row = in + off;
        if (row[2] != (uint8_t)Ns[i] || row[0] != vers[i]) c->bad++;
        off += vrow_len(Ns[i], vers[i]);
        status[i] = verdict(row, in + off - round_len(Ns[i]), Ns[i]);
    }
    if (c->keep_bytes) k.bytes.assign(in, in + off);
    usleep(200);
    std::lock_guard<std::mutex> lk(c->m);
    c->calls.push_back(std::move(k));
    return 0;
}

static int32_t round_runner(bbp_ctx* c, uint32_t R, const uint32_t* round_Ns, const uint8_t* rounds, uint32_t B, const uint32_t* round_of,
                            const uint8_t* rows, int32_t* status, std::string* err) {
    if (B == 0 || B > c->max_batch || R == 0 || R >= B) c->bad++;  // a rounds call shares: fewer rounds than rows
    Call k;
    k.what = 3, k.B = B, k.R = R, k.ns.assign(round_Ns, round_Ns + R), k.round_of.assign(round_of, round_of + B);
    std::vector<size_t> tab_off(R + 1, 0);
    for (uint32_t r = 0; r < R; r++) tab_off[r + 1] = tab_off[r] + round_len(round_Ns[r]);
    size_t off = 0;
    for (uint32_t i = 0; i < B; i++) {
        const uint8_t* row = rows + off;
        if (round_of[i] >= R) {
            c->bad++;
            status[i] = 6;
            continue;
        }
        const uint32_t N = round_Ns[round_of[i]];
        if (row[2] != (uint8_t)N || row[0] != 0) c->bad++;  // compact rows only, and round_of names a round of the row's own length
        status[i] = verdict(row, rounds + tab_off[round_of[i]], N);
        off += short_len(N);
    }
    if (c->keep_bytes) {
        k.bytes.assign(rows, rows + off);
        k.table.assign(rounds, rounds + tab_off[R]);
    }
    usleep(200);
    {
        std::lock_guard<std::mutex> lk(c->m);
        c->calls.push_back(std::move(k));
    }
    if (c->fail_rounds) {
        *err = "stand-in: the rounds call failed";
        return 5;
    }
    return 0;
}

// ---- requests ------------------------------------------------------------------------------------------------------------------
struct Sink {
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
static thread_local uint32_t g_seed = 12345;
static uint8_t rnd() {
    g_seed = g_seed * 1664525u + 1013904223u;
    return (uint8_t)(g_seed >> 24);
}
// seed || pub_list of round `id` with list length N: a function of (id, N) alone
static std::vector<uint8_t> make_round(uint32_t id, uint32_t N) {
    std::vector<uint8_t> v(round_len(N));
    uint32_t s = 2654435761u * (id + 1) + N;
    for (auto& b : v) {
        s = s * 1664525u + 1013904223u;
        b = (uint8_t)(s >> 24);
    }
    return v;
}
static Tagged* make_verify(Sink* s, int index, uint32_t N, uint32_t ver, uint8_t tag, const std::vector<uint8_t>& round) {
    Tagged* t = new Tagged();
    t->sink = s;
    t->index = index;
    t->r.own_in.resize(vrow_len(N, ver));
    for (auto& b : t->r.own_in) b = rnd();
    t->r.own_in[0] = (uint8_t)ver;
    t->r.own_in[1] = tag;
    t->r.own_in[2] = (uint8_t)N;
    memcpy(&t->r.own_in[vrow_len(N, ver) - round_len(N)], round.data(), round_len(N));
    t->r.kind = 1;
    t->r.N = N;
    t->r.rec_ver = ver;
    t->r.in = t->r.own_in.data();
    t->r.in_len = t->r.own_in.size();
    t->r.on_done = hook;
    t->r.user = t;
    t->want = verdict(t->r.in, round.data(), N);
    return t;
}
static void wait_done(Sink& s, int n) {
    std::unique_lock<std::mutex> lk(s.m);
    s.cv.wait(lk, [&] { return s.done >= n; });
}
static void drop(std::vector<Tagged*>& v) {
    for (Tagged* t : v) delete t;
    v.clear();
}

static int g_failed = 0;
static void report(const char* name, bool ok, const std::string& why = "") {
    printf("%s %s%s%s\n", ok ? "PASS" : "FAIL", name, why.empty() ? "" : ": ", why.c_str());
    fflush(stdout);
    if (!ok) g_failed++;
}
static const uint32_t WINDOW_US = 150000;  // long enough that a burst submitted from one thread lands in one window

struct Setup {
    bool runner = true, sharing = true, mixed = true, mixing = true;
    uint32_t max_batch = 4096;
};
static void configure(bbp::Combiner& comb, const Setup& s) {
    if (s.mixed) comb.set_mixed_verify(mixed_runner);
    comb.set_verify_mixing(s.mixing);
    if (s.runner) comb.set_round_verify(round_runner);
    comb.set_round_sharing(s.sharing);
    comb.configure(WINDOW_US, s.max_batch);
}
// the burst `reqs` through a combiner set up as `s`; the round statistics afterwards in st[3]
static void run_burst(bbp_ctx& ctx, Sink& sink, std::vector<Tagged*>& reqs, const Setup& s, uint64_t st[3]) {
    bbp::Combiner comb;
    configure(comb, s);
    for (Tagged* t : reqs)
        if (!comb.submit_async(&ctx, &t->r)) sink.wrong++;
    wait_done(sink, (int)reqs.size());
    comb.round_stats(&st[0], &st[1], &st[2]);
}
// the expanded rows a rounds call stands for: row i || table entry round_of[i]
static std::vector<uint8_t> expand(const Call& c) {
    std::vector<size_t> tab_off(c.R + 1, 0);
    for (uint32_t r = 0; r < c.R; r++) tab_off[r + 1] = tab_off[r] + round_len(c.ns[r]);
    std::vector<uint8_t> out;
    size_t off = 0;
    for (uint32_t i = 0; i < c.B; i++) {
        const uint32_t N = c.ns[c.round_of[i]];
        out.insert(out.end(), c.bytes.begin() + off, c.bytes.begin() + off + short_len(N));
        out.insert(out.end(), c.table.begin() + tab_off[c.round_of[i]], c.table.begin() + tab_off[c.round_of[i] + 1]);
        off += short_len(N);
    }
    return out;
}
static std::vector<uint8_t> queue_bytes(const std::vector<Tagged*>& reqs) {
    std::vector<uint8_t> out;
    for (const Tagged* t : reqs) out.insert(out.end(), t->r.own_in.begin(), t->r.own_in.end());
    return out;
}
static std::string check_statuses(const Sink& sink, const std::vector<Tagged*>& reqs, bool need_varied = true) {
    std::string why;
    bool varied = false;
    for (size_t i = 0; i < reqs.size(); i++) {
        if (sink.results[i].first != reqs[i]->want) why += " request " + std::to_string(i) + " got another row's status;";
        if (reqs[i]->want != reqs[0]->want) varied = true;
    }
    if (need_varied && !varied) why += " (the scenario's statuses are all equal: it shows nothing);";
    return why;
}

// 1. sharing on, one round, 32 requests: one rounds call with R = 1, the table holds the round once, short rows in queue order
static void one_round() {
    bbp_ctx ctx;
    Sink sink;
    std::vector<Tagged*> reqs;
    const uint32_t N = 6;
    const std::vector<uint8_t> round = make_round(1, N);
    for (int i = 0; i < 32; i++) reqs.push_back(make_verify(&sink, i, N, 0, (uint8_t)(3 * i + 1), round));
    uint64_t st[3];
    run_burst(ctx, sink, reqs, Setup{}, st);
    std::string why;
    if (ctx.calls.size() != 1 || ctx.calls[0].what != 3 || ctx.calls[0].B != 32 || ctx.calls[0].R != 1)
        why += " expected one rounds call of 32 rows and one round, got " + std::to_string(ctx.calls.size()) + " call(s);";
    else {
        const Call& c = ctx.calls[0];
        if (c.table != round) why += " the table is not the round, once;";
        if (c.ns != std::vector<uint32_t>{N}) why += " round_Ns;";
        if (c.round_of != std::vector<uint32_t>(32, 0)) why += " round_of;";
        std::vector<uint8_t> want;
        for (Tagged* t : reqs) want.insert(want.end(), t->r.own_in.begin(), t->r.own_in.begin() + short_len(N));
        if (c.bytes != want) why += " rows are not the short rows in queue order;";
    }
    why += check_statuses(sink, reqs);
    if (st[0] != 1 || st[1] != 32 || st[2] != 1) why += " round_stats " + std::to_string(st[0]) + "/" + std::to_string(st[1]) + "/" + std::to_string(st[2]) + ";";
    if (ctx.bad) why += " stand-in saw an inconsistent call;";
    report("one_round_32_requests", why.empty(), why);
    drop(reqs);
}

// 2. three rounds interleaved in queue order, two of them of equal N: numbered by first appearance, table = concatenation, and the
// rows rebuilt from the table are the requests byte for byte
static void three_rounds() {
    bbp_ctx ctx;
    Sink sink;
    std::vector<Tagged*> reqs;
    const uint32_t Ns[3] = {5, 9, 5};  // round ids 0, 1, 2
    const int order[] = {1, 0, 1, 2, 0, 2, 2, 1, 0, 1, 2, 0};  // first appearance: id 1, then 0, then 2
    const uint32_t number[3] = {1, 0, 2};                      // id -> number in the table
    std::vector<std::vector<uint8_t>> rounds;
    for (uint32_t id = 0; id < 3; id++) rounds.push_back(make_round(10 + id, Ns[id]));
    const int n = sizeof order / sizeof order[0];
    for (int i = 0; i < n; i++) reqs.push_back(make_verify(&sink, i, Ns[order[i]], 0, (uint8_t)(5 * i + 2), rounds[order[i]]));
    uint64_t st[3];
    run_burst(ctx, sink, reqs, Setup{}, st);
    std::string why;
    if (ctx.calls.size() != 1 || ctx.calls[0].what != 3 || ctx.calls[0].B != (uint32_t)n || ctx.calls[0].R != 3)
        why += " expected one rounds call with R = 3, got " + std::to_string(ctx.calls.size()) + " call(s);";
    else {
        const Call& c = ctx.calls[0];
        if (c.ns != std::vector<uint32_t>{9, 5, 5}) why += " round_Ns are not in order of first appearance;";
        for (int i = 0; i < n; i++)
            if (c.round_of[i] != number[order[i]]) why += " round_of[" + std::to_string(i) + "];";
        std::vector<uint8_t> tab = rounds[1];
        tab.insert(tab.end(), rounds[0].begin(), rounds[0].end());
        tab.insert(tab.end(), rounds[2].begin(), rounds[2].end());
        if (c.table != tab) why += " the table is not the concatenation of the distinct rounds;";
        if (expand(c) != queue_bytes(reqs)) why += " rows rebuilt from the table differ from the requests;";
    }
    why += check_statuses(sink, reqs);
    if (st[0] != 1 || st[1] != (uint64_t)n || st[2] != 3) why += " round_stats;";
    if (ctx.bad) why += " stand-in saw an inconsistent call;";
    report("three_rounds_interleaved", why.empty(), why);
    drop(reqs);
}

// 3. the hash never decides.  Four requests that all carry the SAME round_hash (set here): round A twice, A with one bit of the last
// list item flipped, A with one bit of the seed flipped -> three rounds.  Conversely equal bytes given DIFFERENT hashes: shared or
// not, each row's round bytes are its own.
static void hash_does_not_decide() {
    const uint32_t N = 4;
    const std::vector<uint8_t> a = make_round(20, N);
    std::vector<uint8_t> item = a, seed = a;
    item[round_len(N) - 1] ^= 0x10;
    seed[0] ^= 0x01;
    std::string why;
    {
        bbp_ctx ctx;
        Sink sink;
        std::vector<Tagged*> reqs;
        const std::vector<uint8_t>* which[] = {&a, &item, &a, &seed, &item};
        for (int i = 0; i < 5; i++) {
            reqs.push_back(make_verify(&sink, i, N, 0, (uint8_t)(i + 1), *which[i]));
            reqs.back()->r.round_hash = 0x1234567887654321ull;
            reqs.back()->r.round_hash_valid = true;
        }
        uint64_t st[3];
        run_burst(ctx, sink, reqs, Setup{}, st);
        if (ctx.calls.size() != 1 || ctx.calls[0].what != 3 || ctx.calls[0].R != 3)
            why += " colliding hashes: expected one rounds call with R = 3;";
        else {
            if (ctx.calls[0].round_of != std::vector<uint32_t>{0, 1, 0, 2, 1}) why += " colliding hashes: round_of;";
            if (expand(ctx.calls[0]) != queue_bytes(reqs)) why += " colliding hashes: a row met another round's bytes;";
        }
        why += check_statuses(sink, reqs, false);
        if (ctx.bad) why += " stand-in saw an inconsistent call;";
        drop(reqs);
    }
    {
        bbp_ctx ctx;
        Sink sink;
        std::vector<Tagged*> reqs;
        for (int i = 0; i < 4; i++) {
            reqs.push_back(make_verify(&sink, i, N, 0, (uint8_t)(i + 9), i == 3 ? item : a));
            reqs.back()->r.round_hash = 1000 + (i == 2 ? 0 : i);  // requests 0 and 2 agree, 1 has the same bytes under another hash
            reqs.back()->r.round_hash_valid = true;
        }
        uint64_t st[3];
        run_burst(ctx, sink, reqs, Setup{}, st);
        std::vector<uint8_t> got;
        for (const Call& c : ctx.calls) {
            if (c.what == 3) {
                const std::vector<uint8_t> e = expand(c);
                got.insert(got.end(), e.begin(), e.end());
            } else
                got.insert(got.end(), c.bytes.begin(), c.bytes.end());
        }
        if (ctx.calls.size() != 1 || got != queue_bytes(reqs)) why += " differing hashes: a row's round bytes are not its own;";
        why += check_statuses(sink, reqs, false);
        if (ctx.bad) why += " stand-in saw an inconsistent call;";
        drop(reqs);
    }
    report("hash_does_not_decide", why.empty(), why);
}

// 4. fallbacks: no rounds call, and the calls recorded are exactly those of the same burst with sharing off
struct Member {
    uint32_t round_id, N, ver;
};
static std::vector<Call> calls_of(const std::vector<Member>& burst, const Setup& s, std::string* why, uint64_t st[3]) {
    bbp_ctx ctx;
    Sink sink;
    std::vector<Tagged*> reqs;
    g_seed = 777;  // the same filler bytes in both runs
    for (size_t i = 0; i < burst.size(); i++)
        reqs.push_back(make_verify(&sink, (int)i, burst[i].N, burst[i].ver, (uint8_t)(7 * i + 3), make_round(burst[i].round_id, burst[i].N)));
    run_burst(ctx, sink, reqs, s, st);
    *why += check_statuses(sink, reqs, false);
    if (ctx.bad) *why += " stand-in saw an inconsistent call;";
    drop(reqs);
    return ctx.calls;
}
static void fallback(const char* name, const std::vector<Member>& burst, Setup on) {
    std::string why;
    uint64_t st[3], st_off[3];
    const std::vector<Call> got = calls_of(burst, on, &why, st);
    Setup off = on;
    off.sharing = false;
    off.runner = true;
    const std::vector<Call> want = calls_of(burst, off, &why, st_off);
    for (const Call& c : got)
        if (c.what == 3) why += " a rounds call was made;";
    if (!(got == want)) why += " the calls differ from those of a run with sharing off (" + std::to_string(got.size()) + " vs " + std::to_string(want.size()) + ");";
    if (want.empty()) why += " no call recorded;";
    if (st[0] || st[1] || st[2] || st_off[0]) why += " the round counters moved;";
    report(name, why.empty(), why);
}
static void fallbacks() {
    std::vector<Member> distinct, shared, two_phase;
    for (uint32_t i = 0; i < 6; i++) distinct.push_back({30 + i, 3 + (i % 3), 0});  // R == B, three list lengths: the mixed call
    for (uint32_t i = 0; i < 8; i++) shared.push_back({40 + (i % 2), 4, 0});         // would share
    two_phase = shared;
    two_phase[5].ver = 1;
    std::vector<Member> distinct_uniform;
    for (uint32_t i = 0; i < 5; i++) distinct_uniform.push_back({50 + i, 4, 0});  // R == B, one list length: the uniform call
    fallback("fallback_all_distinct", distinct, Setup{});
    fallback("fallback_all_distinct_one_n", distinct_uniform, Setup{});
    fallback("fallback_batch_of_one", {{60, 4, 0}}, Setup{});
    fallback("fallback_two_phase_member", two_phase, Setup{});
    Setup no_runner;
    no_runner.runner = false;
    fallback("fallback_no_runner", shared, no_runner);
    Setup sharing_off;
    sharing_off.sharing = false;
    fallback("fallback_sharing_off", shared, sharing_off);
}

// 5. class formation is what it was: with mixing off a batch is one N and layout -- and still shares the rounds of that N
static void classes_with_mixing_off() {
    bbp_ctx ctx;
    Sink sink;
    std::vector<Tagged*> reqs;
    // N = 3: rounds 70, 71 (shared); N = 5: round 72 (shared); N = 5 two-phase: round 72 -> a class of its own, not shared
    const Member burst[] = {{70, 3, 0}, {72, 5, 0}, {71, 3, 0}, {72, 5, 1}, {70, 3, 0}, {72, 5, 0}, {71, 3, 0}, {72, 5, 1}, {72, 5, 0}};
    const int n = sizeof burst / sizeof burst[0];
    for (int i = 0; i < n; i++) reqs.push_back(make_verify(&sink, i, burst[i].N, burst[i].ver, (uint8_t)(11 * i + 1), make_round(burst[i].round_id, burst[i].N)));
    Setup s;
    s.mixing = false;
    uint64_t st[3];
    run_burst(ctx, sink, reqs, s, st);
    std::string why;
    if (ctx.calls.size() != 3) why += " expected three calls (one per list length and layout), got " + std::to_string(ctx.calls.size()) + ";";
    int shared_calls = 0;
    for (const Call& c : ctx.calls) {
        if (c.what == 3) {
            shared_calls++;
            for (uint32_t N : c.ns)
                if (N != c.ns[0]) why += " a rounds call held two list lengths with mixing off;";
            if (!((c.ns[0] == 3 && c.R == 2 && c.B == 4) || (c.ns[0] == 5 && c.R == 1 && c.B == 3))) why += " a rounds call of the wrong shape;";
        } else if (!(c.what == 1 && c.ver == 1 && c.N == 5 && c.B == 2))
            why += " a call that is neither a rounds call nor the two-phase class;";
    }
    if (shared_calls != 2) why += " expected two rounds calls;";
    if (st[0] != 2 || st[1] != 7 || st[2] != 3) why += " round_stats;";
    why += check_statuses(sink, reqs);
    if (ctx.bad) why += " stand-in saw an inconsistent call;";
    report("mixing_off_one_n_still_shares", why.empty(), why);
    drop(reqs);
}

// 6. the rounds call fails: every member gets the call's status and message
static void failing_round_call() {
    bbp_ctx ctx;
    ctx.fail_rounds = true;
    Sink sink;
    std::vector<Tagged*> reqs;
    for (int i = 0; i < 10; i++) {
        reqs.push_back(make_verify(&sink, i, 4 + (i % 2), 0, (uint8_t)(i + 1), make_round(80 + (i % 2), 4 + (i % 2))));
        reqs.back()->want = 5;
    }
    uint64_t st[3];
    run_burst(ctx, sink, reqs, Setup{}, st);
    bool ok = ctx.calls.size() == 1 && ctx.calls[0].what == 3 && !sink.wrong;
    for (int i = 0; i < 10 && ok; i++) ok = sink.results[i].first == 5 && sink.results[i].second == "stand-in: the rounds call failed";
    report("failing_round_call", ok);
    drop(reqs);
}

// 7. max_batch bounds a rounds call as it bounds every other
static void max_batch_is_respected() {
    bbp_ctx ctx;
    ctx.max_batch = 8;
    Sink sink;
    std::vector<Tagged*> reqs;
    for (int i = 0; i < 30; i++) reqs.push_back(make_verify(&sink, i, 4, 0, (uint8_t)(i + 1), make_round(90 + (i % 3), 4)));
    Setup s;
    s.max_batch = 8;
    uint64_t st[3];
    run_burst(ctx, sink, reqs, s, st);
    size_t rows = 0;
    for (const Call& c : ctx.calls) rows += c.B;
    std::string why = check_statuses(sink, reqs);
    if (rows != 30 || ctx.calls.size() < 4) why += " " + std::to_string(ctx.calls.size()) + " call(s), " + std::to_string(rows) + " rows;";
    if (ctx.bad) why += " a call above max_batch or otherwise inconsistent;";
    if (st[0] == 0 || st[2] >= st[1]) why += " nothing was shared;";
    report("max_batch_is_respected", why.empty(), why);
    drop(reqs);
}

// 8. many threads, blocking and asynchronous requests over 5 rounds (two list lengths, now and then a two-phase record), short
// window, small batches, the switch flipped while batches form; one engine and a pool of three
static void stress(int n_targets) {
    std::vector<bbp_ctx> ctxs(n_targets);
    for (auto& c : ctxs) {
        c.max_batch = 8;
        c.keep_bytes = false;
    }
    const int T = 32, PER = 30;
    std::atomic<int> wrong{0};
    Sink sink;
    std::vector<std::vector<Tagged*>> mine(T);
    const uint32_t round_n[5] = {3, 3, 6, 6, 6};
    std::vector<std::vector<uint8_t>> rounds;
    for (uint32_t r = 0; r < 5; r++) rounds.push_back(make_round(100 + r, round_n[r]));
    uint64_t st[3] = {0, 0, 0}, per_target[3] = {0, 0, 0};
    {
        bbp::Combiner comb;
        comb.set_mixed_verify(mixed_runner);
        comb.set_round_verify(round_runner);
        comb.set_round_sharing(true);
        comb.configure(100, 8);
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
                    const uint32_t r = next() % 5, ver = next() % 16 == 0;
                    const int how = next() % 3;  // 0: blocking, 1: asynchronous, 2: blocking with a hash made on this thread, now and then flipping the switch
                    Tagged* t = make_verify(&sink, 0, round_n[r], ver, (uint8_t)next(), rounds[r]);
                    if (how == 2 && comb.round_sharing()) {
                        t->r.round_hash = bbp::hash_bytes(t->r.in + t->r.in_len - bbp::round_bytes(t->r.N), bbp::round_bytes(t->r.N));
                        t->r.round_hash_valid = true;
                    }
                    if (how == 1) {
                        t->index = k * PER + j;
                        mine[k].push_back(t);
                        if (!comb.submit_async(&ctxs[0], &t->r)) wrong++;
                    } else {
                        if (how == 2 && (j % 10) == 0) {  // the switch races with batch formation
                            comb.set_round_sharing(false);
                            comb.set_round_sharing(true);
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
        comb.round_stats(&st[0], &st[1], &st[2]);
        for (int i = 0; i < n_targets; i++) {
            uint64_t a = 0, b = 0, c = 0;
            comb.target_round_stats((size_t)i, &a, &b, &c);
            per_target[0] += a, per_target[1] += b, per_target[2] += c;
        }
    }
    int bad = 0;
    uint64_t round_calls = 0, round_rows = 0, round_tables = 0;
    for (auto& c : ctxs) {
        bad += c.bad;
        for (const Call& k : c.calls)
            if (k.what == 3) round_calls++, round_rows += k.B, round_tables += k.R;
    }
    for (auto& v : mine) drop(v);
    const bool counted = st[0] == round_calls && st[1] == round_rows && st[2] == round_tables && per_target[0] == st[0] && per_target[1] == st[1] &&
                         per_target[2] == st[2];
    const bool ok = !wrong && !sink.wrong && !bad && round_calls > 0 && round_tables < round_rows && counted;
    char name[64];
    snprintf(name, sizeof name, "stress_%d_target%s", n_targets, n_targets > 1 ? "s" : "");
    report(name, ok, ok ? "" : "wrong " + std::to_string(wrong + sink.wrong) + ", bad calls " + std::to_string(bad) + ", rounds calls " + std::to_string(round_calls) +
                                   (counted ? "" : ", counters disagree with the calls seen"));
}

int main(int argc, char** argv) {
    const bool only_stress = argc > 1 && strcmp(argv[1], "stress") == 0;
    if (!only_stress) {
        one_round();
        three_rounds();
        hash_does_not_decide();
        fallbacks();
        classes_with_mixing_off();
        failing_round_call();
        max_batch_is_respected();
    }
    stress(1);
    stress(3);
    printf("RESULT failed %d\n", g_failed);
    return g_failed ? 1 : 0;
}
