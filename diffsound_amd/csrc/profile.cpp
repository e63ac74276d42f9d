// Launch timing hook (bench.py's live roofline figures): while a stream is registered with ds_profile_stream, every launch
// of an ENABLED kind (ds_profile_kinds; default: the fused Chebyshev term only) on it is bracketed by HIP events;
// ds_profile_collect returns the durations with the shape of each launch.  One registered stream at a time; a relaxed flag
// keeps the cost off every other launch.
// Host code only.  Defines ds::ProfScope (ds_common.h); exports ds_profile_stream, ds_profile_kinds, ds_profile_collect.
#include <atomic>
#include <mutex>
#include <vector>

#include "ds_common.h"

namespace {
struct TermRecord {
    hipEvent_t e0, e1;
    int64_t nv, nnzb;
    int ncols, first;  // first | element bytes of the vector blocks << 8 | kind << 16
};
std::atomic<void*> g_prof_stream{nullptr};
std::atomic<unsigned> g_prof_kinds{1u};
std::mutex g_prof_mutex;
std::vector<TermRecord> g_prof_records;
size_t g_prof_cap = 0;
}  // namespace

ds::ProfScope::ProfScope(ds_stream_t stream, int kind, int64_t a, int64_t b, int c, int d) {
    if (stream == nullptr || g_prof_stream.load(std::memory_order_relaxed) != stream) return;
    if (!((g_prof_kinds.load(std::memory_order_relaxed) >> kind) & 1u)) return;
    std::lock_guard<std::mutex> lock(g_prof_mutex);
    if (g_prof_records.size() >= g_prof_cap) return;
    auto* r = new TermRecord{nullptr, nullptr, a, b, c, (d & 0xffff) | (kind << 16)};
    if (hipEventCreate(&r->e0) != hipSuccess) {
        delete r;
        return;
    }
    if (hipEventCreate(&r->e1) != hipSuccess) {
        (void)hipEventDestroy(r->e0);
        delete r;
        return;
    }
    st_ = ds::as_stream(stream);
    (void)hipEventRecord(r->e0, st_);
    rec_ = r;
}

ds::ProfScope::~ProfScope() {
    if (!rec_) return;
    auto* r = static_cast<TermRecord*>(rec_);
    (void)hipEventRecord(r->e1, st_);
    std::lock_guard<std::mutex> lock(g_prof_mutex);
    g_prof_records.push_back(*r);
    delete r;
}

extern "C" int ds_profile_kinds(unsigned mask) {
    g_prof_kinds.store(mask ? mask : 1u);
    return DS_OK;
}

extern "C" int ds_profile_stream(ds_stream_t stream, int64_t capacity) {
    std::lock_guard<std::mutex> lock(g_prof_mutex);
    for (auto& r : g_prof_records) {
        (void)hipEventDestroy(r.e0);
        (void)hipEventDestroy(r.e1);
    }
    g_prof_records.clear();
    g_prof_cap = capacity > 0 ? (size_t)capacity : 0;
    g_prof_stream.store(capacity > 0 ? stream : nullptr);
    return DS_OK;
}

extern "C" int64_t ds_profile_collect(float* ms, int64_t* nv, int64_t* nnzb, int32_t* ncols, int32_t* first, int64_t cap) {
    std::lock_guard<std::mutex> lock(g_prof_mutex);
    g_prof_stream.store(nullptr);
    int64_t n = 0;
    for (auto& r : g_prof_records) {
        if (n < cap && hipEventSynchronize(r.e1) == hipSuccess) {
            float t = 0.f;
            if (hipEventElapsedTime(&t, r.e0, r.e1) == hipSuccess) {
                ms[n] = t, nv[n] = r.nv, nnzb[n] = r.nnzb, ncols[n] = r.ncols, first[n] = r.first;
                ++n;
            }
        }
        (void)hipEventDestroy(r.e0);
        (void)hipEventDestroy(r.e1);
    }
    g_prof_records.clear();
    return n;
}
