// handle_owner_main.cpp -- the ownership rules of csrc/tmvb_handle.h, checked on the host against a stub HIP runtime (no HIP library is linked, no
// device is opened).  Built and run by tests/test_handle_owner_host.py:
//     g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I<rocm>/include -I include -I topicmodelsvb.jl_amd/csrc -fsanitize=address,undefined
//
// One representative handle life -- twelve allocations, six events (three of them in a std::vector), four auxiliary streams, a regrown buffer, a
// statistics buffer given up for one the host bound, the globals and two of the streams given up for another handle's, every event remade, release,
// release again -- runs once without a fault and once per creating call of the sequence with that call failing, as the create guard meets it: the
// build stops there and the handle is released as far as it got.  The stubs log every call and know what is live; whatever the handle only uses
// (the bound buffer, the other handle's globals and streams) must still be there at the end.
#include "tmvb_handle.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>

// ---------------------------------------------------------------------------------------------------------------- stub runtime
enum kind { SET_DEVICE, MALLOC, FREE, EVENT_CREATE, EVENT_DESTROY, STREAM_CREATE, STREAM_RELEASE, SYNC, RELEASE_BEGIN };
struct entry { kind k; void* what; };

static std::vector<entry> g_log;
static std::set<void*> g_live_mem, g_live_ev, g_live_st, g_foreign;
static int g_calls, g_fail_at, g_errors;                // g_calls counts the creating calls, the ones that can be made to fail
static kind g_failed_kind;
static std::string g_last_error;

static void complain(const char* what)
{
    fprintf(stderr, "  stub: %s (injected failure at call %d)\n", what, g_fail_at);
    g_errors++;
}

static bool inject(kind k)
{
    if (g_calls++ != g_fail_at) return false;
    g_failed_kind = k;
    return true;
}

void tmvb_set_error(const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
}

hipStream_t tmvb_pool_stream(int, int, bool)
{
    if (inject(STREAM_CREATE)) return nullptr;
    void* s = malloc(1);
    g_live_st.insert(s);
    g_log.push_back({STREAM_CREATE, s});
    return (hipStream_t)s;
}
void tmvb_release_stream(hipStream_t st)
{
    g_log.push_back({STREAM_RELEASE, st});
    if (g_foreign.count(st)) { complain("a borrowed stream was released"); return; }
    if (!g_live_st.erase(st)) { complain("release of a stream that is not live"); return; }
    free(st);
}

extern "C" {
hipError_t hipSetDevice(int) { g_log.push_back({SET_DEVICE, nullptr}); return hipSuccess; }
hipError_t hipMalloc(void** p, size_t n)
{
    if (inject(MALLOC)) return hipErrorOutOfMemory;
    if (n == 0) complain("hipMalloc of zero bytes");
    *p = malloc(n);
    g_live_mem.insert(*p);
    g_log.push_back({MALLOC, *p});
    return hipSuccess;
}
hipError_t hipFree(void* p)
{
    g_log.push_back({FREE, p});
    if (g_foreign.count(p)) { complain("hipFree of memory the handle does not own"); return hipErrorInvalidValue; }
    if (!g_live_mem.erase(p)) { complain("hipFree of memory that is not live"); return hipErrorInvalidValue; }
    free(p);
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned)
{
    if (inject(EVENT_CREATE)) return hipErrorUnknown;
    *e = (hipEvent_t)malloc(1);
    g_live_ev.insert(*e);
    g_log.push_back({EVENT_CREATE, *e});
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e)
{
    g_log.push_back({EVENT_DESTROY, e});
    if (!g_live_ev.erase(e)) { complain("hipEventDestroy of an event that is not live"); return hipErrorInvalidValue; }
    free(e);
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s)
{
    g_log.push_back({SYNC, s});
    if (s && !g_live_st.count(s) && !g_foreign.count(s)) complain("hipStreamSynchronize of a stream that is not live");
    return hipSuccess;
}
const char* hipGetErrorString(hipError_t) { return "stub error"; }
}

// ---------------------------------------------------------------------------------------------------------------- the handle under test
static const int NAUX = 4;
struct handle {
    float* d_globals[2] = {nullptr, nullptr};
    float* d_stats = nullptr;
    double* d_logz = nullptr;
    char* d_empty = nullptr;
    int* d_state[7] = {};
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_fork = nullptr;
    std::vector<hipEvent_t> ev_piece;
    hipStream_t aux[NAUX] = {};
    tmvb_owned mem;
};

// what another handle, or the host, owns
static float* f_globals[2];
static float* f_stats;
static hipStream_t f_aux[2];
static hipStream_t const ctx_stream = nullptr;          // the context's stream: the null stream will do

static int build(handle& h)
{
    int rc;
    if ((rc = h.mem.alloc(&h.d_globals[0], 64)) || (rc = h.mem.alloc(&h.d_globals[1], 64)) || (rc = h.mem.alloc(&h.d_stats, 32)) ||
        (rc = h.mem.alloc(&h.d_logz, 8)) || (rc = h.mem.alloc(&h.d_empty, 0)))          // an empty array still gets an address
        return rc;
    for (int*& p : h.d_state) if ((rc = h.mem.alloc(&p, 16))) return rc;
    if ((rc = h.mem.event(&h.ev0, hipEventDefault)) || (rc = h.mem.event(&h.ev1, hipEventDefault)) || (rc = h.mem.event(&h.ev_fork, hipEventDisableTiming))) return rc;
    h.ev_piece.assign(3, nullptr);
    for (hipEvent_t& e : h.ev_piece) if ((rc = h.mem.event(&e, hipEventDisableTiming))) return rc;
    for (int a = 0; a < NAUX; a++) if ((rc = h.mem.aux(&h.aux[a], 0, 1 + a, a == 1))) return rc;
    // a buffer regrown in place
    h.mem.drop(&h.d_logz);
    if ((rc = h.mem.alloc(&h.d_logz, 64))) return rc;
    // tmvb_*_bind_stats: the own statistics buffer goes, the host's is adopted
    h.mem.drop(&h.d_stats);
    h.d_stats = f_stats;
    h.mem.drop(&h.d_stats);                             // bound, not owned: nothing happens
    if (h.d_stats != f_stats) complain("dropping a bound pointer changed it");
    // tmvb_*_share_globals: the own globals and two of the streams go, another handle's are used from here on
    for (int q = 0; q < 2; q++) { h.mem.drop(&h.d_globals[q]); h.d_globals[q] = f_globals[q]; }
    for (int a = 2; a < NAUX; a++) h.mem.borrow(&h.aux[a], f_aux[a - 2]);
    // tmvb_lda_set_comm: every ordering event again, with other flags
    for (hipEvent_t* e : {&h.ev0, &h.ev1, &h.ev_fork}) if ((rc = h.mem.remake(e, hipEventDefault))) return rc;
    for (hipEvent_t& e : h.ev_piece) if ((rc = h.mem.remake(&e, hipEventDefault))) return rc;
    return TMVB_OK;
}

// ---------------------------------------------------------------------------------------------------------------- checks
static int g_failures;
#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "FAIL (injected failure at call %d): ", g_fail_at); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); g_failures++; } } while (0)

static int count(kind k, size_t from = 0) { int n = 0; for (size_t i = from; i < g_log.size(); i++) n += g_log[i].k == k; return n; }

static int attempt(int fail_at)
{
    g_log.clear(); g_calls = 0; g_errors = 0; g_fail_at = fail_at; g_last_error.clear();
    int rc;
    {
        handle h;
        rc = build(h);
        const int own_streams = (int)g_live_st.size(), seen_streams = (int)h.mem.streams.size();
        g_log.push_back({RELEASE_BEGIN, nullptr});
        const size_t begin = g_log.size();
        h.mem.release(0, ctx_stream);
        // the waits -- every stream the handle issues on, then the context's -- in front of the first release
        size_t first_release = g_log.size(), last_sync = begin;
        for (size_t i = begin; i < g_log.size(); i++) {
            const kind k = g_log[i].k;
            if ((k == FREE || k == EVENT_DESTROY || k == STREAM_RELEASE) && i < first_release) first_release = i;
            if (k == SYNC) last_sync = i;
        }
        if (g_log.size() > begin) {
            CHECK(g_log[begin].k == SET_DEVICE, "release does not set the device first");
            CHECK(count(SYNC, begin) == seen_streams + 1, "%d stream waits in release, %d streams and the context's expected", count(SYNC, begin), seen_streams);
            CHECK(last_sync < first_release, "a release at log position %zu, the last wait is at %zu", first_release, last_sync);
            CHECK(g_log[last_sync].what == (void*)ctx_stream, "the last wait is not for the context's stream");
            CHECK(count(STREAM_RELEASE, begin) == own_streams, "%d streams given back in release, %d are the handle's own", count(STREAM_RELEASE, begin), own_streams);
        }
        // everything the handle made is gone, each once (the stubs complain about a second time); what it only used is untouched
        CHECK(g_live_mem.empty() && g_live_ev.empty() && g_live_st.empty(), "%zu allocations, %zu events, %zu streams left", g_live_mem.size(), g_live_ev.size(), g_live_st.size());
        CHECK(count(MALLOC) == count(FREE) && count(EVENT_CREATE) == count(EVENT_DESTROY) && count(STREAM_CREATE) == count(STREAM_RELEASE),
              "%d / %d allocations, %d / %d events, %d / %d streams released", count(FREE), count(MALLOC), count(EVENT_DESTROY), count(EVENT_CREATE),
              count(STREAM_RELEASE), count(STREAM_CREATE));
        const size_t after = g_log.size();
        h.mem.release(0, ctx_stream);
        CHECK(g_log.size() == after, "a second release made %zu calls", g_log.size() - after);
    }
    CHECK(g_errors == 0, "%d complaints of the stub runtime", g_errors);
    return rc;
}

int main()
{
    for (float*& p : f_globals) { p = (float*)malloc(4); g_foreign.insert(p); }
    f_stats = (float*)malloc(4); g_foreign.insert(f_stats);
    for (hipStream_t& s : f_aux) { s = (hipStream_t)malloc(1); g_foreign.insert(s); }

    // ---- no fault
    int rc = attempt(-1);
    const int n_calls = g_calls;
    CHECK(rc == TMVB_OK, "rc = %d", rc);
    CHECK(count(MALLOC) == 13 && count(EVENT_CREATE) == 12 && count(STREAM_CREATE) == 4, "%d allocations, %d events, %d streams made", count(MALLOC), count(EVENT_CREATE), count(STREAM_CREATE));
    CHECK(n_calls == 29, "the sequence has %d creating calls, 29 expected", n_calls);

    // ---- one run per creating call of the sequence, with that call failing
    for (int f = 0; f < n_calls; f++) {
        rc = attempt(f);
        CHECK(g_calls == f + 1, "the build went on after the failing call");
        const int want = g_failed_kind == MALLOC ? TMVB_ENOMEM : TMVB_EHIP;
        CHECK(rc == want, "rc = %d, injected %d", rc, want);
        CHECK(!g_last_error.empty(), "no error message");
    }
    CHECK(g_foreign.size() == 5, "foreign objects lost");
    for (void* p : g_foreign) free(p);
    if (g_failures) { fprintf(stderr, "%d checks failed\n", g_failures); return 1; }
    printf("handle owner ok: %d injected failures and the success path\n", n_calls);
    return 0;
}
