// call_scope_main.cpp -- the release order of csrc/tmvb_call.h, checked on the host against a stub HIP runtime (no HIP library is linked, no device
// is opened).  Built and run by tests/test_call_scope_host.py:
//     g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I<rocm>/include -I include -I topicmodelsvb.jl_amd/csrc -fsanitize=address,undefined
//
// The stubs log every call; asynchronous copies are only carried out at hipStreamSynchronize, so a buffer released while a copy is pending is
// read or written after its free (the sanitizer reports it) and is flagged by the stub as well.  One representative call -- two events, three
// allocations, one upload, one malloc'd result buffer under the guard, one staging buffer -- runs once without a fault and once per HIP call of
// the sequence with that call made to fail.
#include "tmvb_call.h"

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>

// ---------------------------------------------------------------------------------------------------------------- stub runtime
enum kind { SET_DEVICE, EVENT_CREATE, EVENT_DESTROY, EVENT_RECORD, EVENT_ELAPSED, MALLOC, FREE, MEMCPY, SYNC, RESULT_FREE, STAGING_GONE };
struct copy { void* dst; const void* src; size_t bytes; };

static std::vector<kind> g_log;
static std::vector<copy> g_pending;                     // copies issued and not yet waited for
static std::set<void*> g_live_mem, g_live_ev;
static int g_calls, g_fail_at, g_errors;                // g_calls counts the calls that can be made to fail
static kind g_failed_kind;
static int g_failed_pos;                                // position in g_log of the call that failed
static std::string g_last_error;

static void complain(const char* what)
{
    fprintf(stderr, "  stub: %s (injected failure at call %d)\n", what, g_fail_at);
    g_errors++;
}

static bool inject(kind k)
{
    g_log.push_back(k);
    if (g_calls++ != g_fail_at) return false;
    g_failed_kind = k;
    g_failed_pos = (int)g_log.size() - 1;
    return true;
}

static void release(kind k)
{
    if (!g_pending.empty()) complain("a release while copies are pending on the stream");
    g_log.push_back(k);
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

extern "C" {
hipError_t hipSetDevice(int) { return inject(SET_DEVICE) ? hipErrorInvalidDevice : hipSuccess; }
hipError_t hipMalloc(void** p, size_t n)
{
    *p = nullptr;
    if (inject(MALLOC)) return hipErrorOutOfMemory;
    *p = malloc(n);
    g_live_mem.insert(*p);
    return hipSuccess;
}
hipError_t hipFree(void* p)
{
    release(FREE);
    if (!g_live_mem.erase(p)) { complain("hipFree of memory that is not live"); return hipErrorInvalidValue; }
    free(p);
    return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t* e)
{
    if (inject(EVENT_CREATE)) return hipErrorUnknown;
    *e = (hipEvent_t)malloc(1);
    g_live_ev.insert(*e);
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e)
{
    release(EVENT_DESTROY);
    if (!g_live_ev.erase(e)) { complain("hipEventDestroy of an event that is not live"); return hipErrorInvalidValue; }
    free(e);
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t)
{
    if (!g_live_ev.count(e)) complain("hipEventRecord of an event that is not live");
    return inject(EVENT_RECORD) ? hipErrorUnknown : hipSuccess;
}
hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b)
{
    if (!g_live_ev.count(a) || !g_live_ev.count(b)) complain("hipEventElapsedTime of an event that is not live");
    if (inject(EVENT_ELAPSED)) return hipErrorUnknown;
    *ms = 1.0f;
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind, hipStream_t)
{
    if (inject(MEMCPY)) return hipErrorUnknown;
    g_pending.push_back({dst, src, bytes});
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t)
{
    for (const copy& c : g_pending) memcpy(c.dst, c.src, c.bytes);
    g_pending.clear();
    return inject(SYNC) ? hipErrorUnknown : hipSuccess;
}
const char* hipGetErrorString(hipError_t) { return "stub error"; }
}

// ---------------------------------------------------------------------------------------------------------------- the call under test
struct result_t { int32_t* values; int64_t n; };
static void result_free(result_t* r)
{
    release(RESULT_FREE);
    free(r->values);
    memset(r, 0, sizeof(*r));
}
struct staging {                                        // a std::vector that says when it goes
    std::vector<int32_t> v;
    ~staging() { release(STAGING_GONE); }
};

static const int N = 16;

static int run_call(result_t* out, float* ms)
{
    tmvb_result_guard<result_t, result_free> guard{out};
    staging h_in{std::vector<int32_t>(N, 7)};
    hipStream_t st = nullptr;
    tmvb_call c("scope_test", 0, st);
    TMVB_CALL_TRY(c, c.begin());
    TMVB_CALL_TRY(c, c.events(2));
    int32_t *d_a, *d_b, *d_in;
    char* d_tmp;
    TMVB_CALL_TRY(c, c.alloc(&d_a, N));
    TMVB_CALL_TRY(c, c.alloc(&d_b, 0));                 // an empty array still gets an address
    TMVB_CALL_TRY(c, c.alloc(&d_tmp, 64));
    TMVB_CALL_TRY(c, c.upload(&d_in, (const int32_t*)h_in.v.data(), N));
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(0), st));
    TMVB_CALL_HIP(c, hipEventRecord(c.ev(1), st));
    out->n = N;
    TMVB_CALL_TRY(c, tmvb_host_alloc("scope_test", &out->values, N));
    TMVB_CALL_HIP(c, hipMemcpyAsync(out->values, d_in, N * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    TMVB_CALL_HIP(c, hipStreamSynchronize(st));         // the call's own wait
    TMVB_CALL_TRY(c, c.elapsed(ms, 0, 1));
    guard.release();
    return TMVB_OK;
}

// ---------------------------------------------------------------------------------------------------------------- checks
static int g_failures;
#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "FAIL (injected failure at call %d): ", g_fail_at); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); g_failures++; } } while (0)

static int count(kind k) { int n = 0; for (kind x : g_log) n += x == k; return n; }
static int first_of(std::initializer_list<kind> ks) { for (size_t i = 0; i < g_log.size(); i++) for (kind k : ks) if (g_log[i] == k) return (int)i; return -1; }
static int last_of(kind k) { for (int i = (int)g_log.size() - 1; i >= 0; i--) if (g_log[(size_t)i] == k) return i; return -1; }

static int attempt(int fail_at, result_t* out, float* ms)
{
    g_log.clear(); g_pending.clear(); g_calls = 0; g_errors = 0; g_fail_at = fail_at; g_failed_pos = -1; g_last_error.clear();
    memset(out, 0, sizeof(*out));
    const int rc = run_call(out, ms);
    CHECK(g_errors == 0, "%d complaints of the stub runtime", g_errors);
    CHECK(g_pending.empty(), "copies still pending after the call");
    return rc;
}

int main()
{
    result_t out;
    float ms = 0.0f;
    // ---- no fault: every allocation and event released once, no wait beyond the call's own, the data went through
    int rc = attempt(-1, &out, &ms);
    const int n_calls = g_calls;
    CHECK(rc == TMVB_OK, "rc = %d", rc);
    CHECK(count(SYNC) == 1, "%d stream synchronisations on the success path, the call has 1", count(SYNC));
    CHECK(count(MALLOC) == 4 && count(FREE) == 4 && count(EVENT_CREATE) == 2 && count(EVENT_DESTROY) == 2, "%d / %d allocations, %d / %d events released",
          count(FREE), count(MALLOC), count(EVENT_DESTROY), count(EVENT_CREATE));
    CHECK(g_live_mem.empty() && g_live_ev.empty(), "device memory or events left");
    CHECK(count(RESULT_FREE) == 0 && out.values != nullptr && out.n == N, "the result of a successful call was freed");
    CHECK(first_of({FREE, EVENT_DESTROY}) > last_of(SYNC), "a release in front of the call's own wait");
    for (int i = 0; out.values && i < N; i++) CHECK(out.values[i] == 7, "values[%d] = %d", i, out.values[i]);
    CHECK(ms == 1.0f, "ms = %g", ms);
    free(out.values);
    CHECK(n_calls == 13, "the sequence has %d HIP calls that can fail, 13 expected", n_calls);

    // ---- one run per HIP call of the sequence, with that call failing
    for (int f = 0; f < n_calls; f++) {
        rc = attempt(f, &out, &ms);
        CHECK(g_failed_pos >= 0, "no call failed");
        const int want = g_failed_kind == MALLOC ? TMVB_ENOMEM : TMVB_EHIP;
        CHECK(rc == want, "rc = %d, injected %d", rc, want);
        CHECK(!g_last_error.empty(), "no error message");
        int ok_mem = 0, ok_ev = 0;
        for (int i = 0; i < (int)g_log.size(); i++) {
            if (i == g_failed_pos) continue;
            ok_mem += g_log[(size_t)i] == MALLOC; ok_ev += g_log[(size_t)i] == EVENT_CREATE;
        }
        CHECK(count(FREE) == ok_mem && count(EVENT_DESTROY) == ok_ev, "%d of %d allocations, %d of %d events released", count(FREE), ok_mem, count(EVENT_DESTROY), ok_ev);
        CHECK(g_live_mem.empty() && g_live_ev.empty(), "device memory or events left");
        // fail() waits for the stream right after the failing call, in front of every release
        CHECK((size_t)g_failed_pos + 1 < g_log.size() && g_log[(size_t)g_failed_pos + 1] == SYNC, "no stream synchronisation right after the failing call");
        const int first_release = first_of({FREE, EVENT_DESTROY, RESULT_FREE, STAGING_GONE});
        CHECK(first_release > g_failed_pos + 1, "a release at log position %d, the wait is at %d", first_release, g_failed_pos + 1);
        // device memory first, then the staging buffer and the result struct
        CHECK(count(RESULT_FREE) == 1 && count(STAGING_GONE) == 1, "result freed %d times, staging %d times", count(RESULT_FREE), count(STAGING_GONE));
        const int last_dev = std::max(last_of(FREE), last_of(EVENT_DESTROY));
        CHECK(last_of(RESULT_FREE) > last_dev && last_of(STAGING_GONE) > last_dev, "host memory released in front of device memory");
        CHECK(out.values == nullptr, "the result struct still holds a buffer");
    }
    if (g_failures) { fprintf(stderr, "%d checks failed\n", g_failures); return 1; }
    printf("call scope ok: %d injected failures and the success path\n", n_calls);
    return 0;
}
