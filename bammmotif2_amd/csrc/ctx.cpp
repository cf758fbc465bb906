// Contexts of the C ABI (include/bamm_em.h): a device and a stream, the pinned staging area every large transfer between
// the caller's memory and the device goes through, the scratch pool that hands set-sized blocks from one handle to the next.
// Host code only.

#include <atomic>
#include <climits>
#include <type_traits>
#include <variant>

#include "handles.h"

namespace bamm {

constexpr size_t kScratchMinBytes = size_t(4) << 20;         // smaller blocks are plain allocations
static std::mutex g_ctx_mu;
static std::vector<bamm_ctx*> g_ctxs;                                // live contexts (flush_idle_scratch walks them)
// device blocks handed to an owner (dev_alloc_bytes, scratch_alloc_bytes) and not yet taken back (scratch_free); a pool's
// idle blocks are nobody's.  Read by bamm_device_blocks_live alone: the tests' check that a handle returned all it took.
static std::atomic<long long> g_blocks_live{0};

static bool flush_idle_scratch(int device) {
    bool any = false;
    std::lock_guard<std::mutex> g(g_ctx_mu);
    for (bamm_ctx* c : g_ctxs) {
        if (c->device != device) continue;
        std::lock_guard<std::mutex> l(c->scratch_mu);
        for (auto& b : c->scratch_idle) { (void)hipFree(b.first); any = true; }
        c->scratch_idle.clear();
        c->scratch_idle_bytes = 0;
    }
    return any;
}

int dev_alloc_bytes(void** p, size_t bytes) {
    *p = nullptr;
    hipError_t e = hipMalloc(p, bytes ? bytes : 1);
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        int device = 0;
        (void)hipGetDevice(&device);
        if (flush_idle_scratch(device)) e = hipMalloc(p, bytes ? bytes : 1);
    }
    if (e != hipSuccess) {
        set_error("hipMalloc of %zu bytes failed: %s", bytes, hipGetErrorString(e));
        *p = nullptr;
        return BAMM_ERR_HIP;
    }
    g_blocks_live++;
    return BAMM_OK;
}

constexpr size_t kStageChunk = size_t(4) << 20;               // bytes per pinned chunk (two of them: 8 MB pinned per context, 1.5 ms to allocate)
constexpr size_t kStageMin = size_t(64) << 10;                // smaller transfers: the runtime copies them through its own staging buffer

// memcpy on the host threads the process was granted (a chunk of 8 MB: 0.9 ms on one thread, 0.2 ms on eight)
void par_memcpy(void* dst, const void* src, size_t bytes) {
    const uint32_t T = (uint32_t)std::max<size_t>(1, std::min<size_t>(host_threads_hint(), bytes >> 20));
    if (T <= 1) { memcpy(dst, src, bytes); return; }
    std::vector<std::thread> th;
    for (uint32_t t = 0; t < T; t++) {
        const size_t b = bytes * t / T & ~size_t(63), e = t + 1 == T ? bytes : (bytes * (t + 1) / T & ~size_t(63));
        th.emplace_back([=] { memcpy((unsigned char*)dst + b, (const unsigned char*)src + b, e - b); });
    }
    for (auto& x : th) x.join();
}

static int stage_ready(bamm_ctx* c) {                         // stage_mu held
    if (c->stage_buf[0]) return BAMM_OK;
    unsigned char* p = nullptr;
    if (hipHostMalloc((void**)&p, 2 * kStageChunk, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        set_error("hipHostMalloc of the %zu-byte staging area failed", 2 * kStageChunk);
        return BAMM_ERR_HIP;
    }
    for (hipEvent_t& e : c->stage_ev)
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { (void)hipHostFree(p); set_error("hipEventCreate failed"); return BAMM_ERR_HIP; }
    c->stage_buf[0] = p; c->stage_buf[1] = p + kStageChunk;
    return BAMM_OK;
}

// host -> device on the context's stream.  Returns when `src` has been read (the caller may free it); the copies themselves
// are ordered on the stream like any other work.
int ctx_upload(bamm_ctx* c, void* dst_dev, const void* src, size_t bytes) {
    if (!bytes) return BAMM_OK;
    if (bytes < kStageMin) { BAMM_HIP(hipMemcpyAsync(dst_dev, src, bytes, hipMemcpyHostToDevice, c->stream)); return BAMM_OK; }
    std::lock_guard<std::mutex> l(c->stage_mu);
    if (int rc = stage_ready(c)) return rc;
    uint32_t b = 0;
    for (size_t at = 0; at < bytes; at += kStageChunk, b ^= 1u) {
        const size_t len = std::min(kStageChunk, bytes - at);
        if (c->stage_used[b]) BAMM_HIP(hipEventSynchronize(c->stage_ev[b]));      // the copy that last read this chunk is done
        par_memcpy(c->stage_buf[b], (const unsigned char*)src + at, len);
        BAMM_HIP(hipMemcpyAsync((unsigned char*)dst_dev + at, c->stage_buf[b], len, hipMemcpyHostToDevice, c->stream));
        BAMM_HIP(hipEventRecord(c->stage_ev[b], c->stream));
        c->stage_used[b] = true;
    }
    return BAMM_OK;
}

// device -> host on the context's stream.  Returns when `dst` holds the data (everything enqueued on the stream before it
// has completed by then).  Small transfers are enqueued only, like a hipMemcpyAsync: the caller synchronises.
int ctx_download(bamm_ctx* c, void* dst, const void* src_dev, size_t bytes) {
    if (!bytes) return BAMM_OK;
    if (bytes < kStageMin) { BAMM_HIP(hipMemcpyAsync(dst, src_dev, bytes, hipMemcpyDeviceToHost, c->stream)); return BAMM_OK; }
    std::lock_guard<std::mutex> l(c->stage_mu);
    if (int rc = stage_ready(c)) return rc;
    for (uint32_t b = 0; b < 2u; b++)
        if (c->stage_used[b]) { BAMM_HIP(hipEventSynchronize(c->stage_ev[b])); c->stage_used[b] = false; }
    const size_t chunks = (bytes + kStageChunk - 1) / kStageChunk;
    for (size_t i = 0; i <= chunks; i++) {                   // chunk i is enqueued while chunk i - 1 is copied out
        if (i < chunks) {
            const size_t at = i * kStageChunk, len = std::min(kStageChunk, bytes - at);
            BAMM_HIP(hipMemcpyAsync(c->stage_buf[i & 1u], (const unsigned char*)src_dev + at, len, hipMemcpyDeviceToHost, c->stream));
            BAMM_HIP(hipEventRecord(c->stage_ev[i & 1u], c->stream));
        }
        if (i > 0) {
            const size_t at = (i - 1) * kStageChunk, len = std::min(kStageChunk, bytes - at);
            BAMM_HIP(hipEventSynchronize(c->stage_ev[(i - 1) & 1u]));
            par_memcpy((unsigned char*)dst + at, c->stage_buf[(i - 1) & 1u], len);
        }
    }
    return BAMM_OK;
}

int scratch_alloc_bytes(bamm_ctx* c, void** p, size_t bytes) {
    *p = nullptr;
    if (bytes < kScratchMinBytes) return dev_alloc_bytes(p, bytes);
    bytes = (bytes + (size_t(2) << 20) - 1) & ~((size_t(2) << 20) - 1);
    void* got = nullptr;
    size_t got_bytes = 0;
    {
        std::lock_guard<std::mutex> l(c->scratch_mu);
        size_t best = (size_t)-1;
        for (size_t i = 0; i < c->scratch_idle.size(); i++) {   // the tightest idle block of at most twice the size
            const size_t b = c->scratch_idle[i].second;
            if (b >= bytes && b <= 2 * bytes && (best == (size_t)-1 || b < c->scratch_idle[best].second)) best = i;
        }
        if (best != (size_t)-1) {
            got = c->scratch_idle[best].first; got_bytes = c->scratch_idle[best].second;
            c->scratch_idle.erase(c->scratch_idle.begin() + (ptrdiff_t)best);
            c->scratch_idle_bytes -= got_bytes;
            c->scratch_hits++;
        } else {
            c->scratch_misses++;
        }
    }
    if (!got) {
        if (int rc = dev_alloc_bytes(&got, bytes)) return rc;
        got_bytes = bytes;
    } else {
        g_blocks_live++;                                     // (a block that was idle; dev_alloc_bytes counted the others)
    }
    if (c->scratch_poison && hipMemsetAsync(got, 0xff, got_bytes, c->stream) != hipSuccess) {
        (void)hipFree(got);
        g_blocks_live--;
        set_error("hipMemsetAsync failed");
        return BAMM_ERR_HIP;
    }
    {
        std::lock_guard<std::mutex> l(c->scratch_mu);
        c->scratch_live[got] = got_bytes;
    }
    *p = got;
    return BAMM_OK;
}

// Returns a block to its context (the caller has made sure that nothing enqueued on OTHER streams still uses it;
// work on the context's own stream is ordered before the next owner's).  Plain allocations are freed.
void scratch_free(bamm_ctx* c, void* p) {
    if (!p) return;
    g_blocks_live--;
    std::vector<void*> evict;
    {
        std::lock_guard<std::mutex> l(c->scratch_mu);
        auto it = c->scratch_live.find(p);
        if (it == c->scratch_live.end()) {
            evict.push_back(p);
        } else {
            c->scratch_idle.emplace_back(p, it->second);
            c->scratch_idle_bytes += it->second;
            c->scratch_live.erase(it);
            while (c->scratch_idle_bytes > c->scratch_cap_bytes && !c->scratch_idle.empty()) {     // oldest first
                evict.push_back(c->scratch_idle.front().first);
                c->scratch_idle_bytes -= c->scratch_idle.front().second;
                c->scratch_idle.erase(c->scratch_idle.begin());
            }
        }
    }
    for (void* q : evict) (void)hipFree(q);
}

// a process may drive several devices (one context each): make the context's device current
int use_device(const bamm_ctx* c) {
    BAMM_HIP(hipSetDevice(c->device));
    return BAMM_OK;
}
int ctx_device(const bamm_ctx* c) { return c->device; }
hipStream_t ctx_stream(const bamm_ctx* c) { return c->stream; }

}  // namespace bamm

using namespace bamm;

namespace {

// BAMM_ERR_NO_DEVICE without a visible device (bamm_device_count), BAMM_ERR_ARG when `device` or `peer` is not one of them
int check_device_index(int device, int peer) {
    int count = 0;
    if (int rc = bamm_device_count(&count)) return rc;
    if (device < 0 || device >= count) { set_error("device %d out of range (0..%d)", device, count - 1); return BAMM_ERR_ARG; }
    if (peer < 0 || peer >= count) { set_error("peer %d out of range (0..%d)", peer, count - 1); return BAMM_ERR_ARG; }
    return BAMM_OK;
}

// bamm_ctx_set_tuning's keys and the context field each one sets.  A switch takes any value (non-zero = on); a number
// must lie in lo..hi or be `also`.  scratch_cache_mb = 0 also releases the idle scratch blocks at once.
struct TuningKey {
    const char* key;
    std::variant<bool bamm_ctx::*, uint32_t bamm_ctx::*, int bamm_ctx::*, size_t bamm_ctx::*> field;
    int lo = 0, hi = 0, also = 0;
    const char* range = nullptr;                             // what a refusal says (nullptr: a switch)
};
const TuningKey kTuningKeys[] = {
    {"grouped", &bamm_ctx::use_grouped},
    {"sparse", &bamm_ctx::use_sparse},
    {"e_fused", &bamm_ctx::use_e_fused},
    {"e_list", &bamm_ctx::use_e_list},
    {"fused_update", &bamm_ctx::use_fused_update},
    {"adaptive_lists", &bamm_ctx::use_adaptive_lists},
    {"update_blocks", &bamm_ctx::use_update_blocks},
    {"score_tiles", &bamm_ctx::use_score_tiles},
    {"score_slices", &bamm_ctx::use_score_slices},
    {"em_tiles", &bamm_ctx::use_em_tiles},
    {"mix_anchor", &bamm_ctx::use_mix_anchor},
    {"scratch_poison", &bamm_ctx::scratch_poison},
    {"peer_allreduce", &bamm_ctx::use_peer_allreduce},
    {"peer_timeout_ms", &bamm_ctx::peer_timeout_ms, 1, 600000, 1, "1..600000"},
    {"scratch_cache_mb", &bamm_ctx::scratch_cap_bytes, 0, INT_MAX, 0, ">= 0"},
    {"list_threshold_pct", &bamm_ctx::list_threshold_pct, 0, 100, 0, "0..100"},
    {"sites_chunk_positions", &bamm_ctx::sites_chunk_positions, 0, INT_MAX, 0, ">= 0"},
    {"neg_segment_positions", &bamm_ctx::neg_segment_positions, 16, 1 << 20, 0, "0 (default) or 16..1048576"},
    {"kmer_segment_positions", &bamm_ctx::kmer_segment_positions, 16, 1 << 20, 0, "0 (default) or 16..1048576"},
    {"kmer_flush_windows", &bamm_ctx::kmer_flush_windows, 1, INT_MAX, 0, "0 (default) or >= 1"},
    {"group_size", &bamm_ctx::group_size, 2, 4, 0, "0 (auto) or 2..4"},
    {"group_layout", &bamm_ctx::group_layout, -1, 3, 8, "-1 (auto), 0..3 or 8 (mixed rows)"},
};

}  // namespace

extern "C" {

// ------------------------------------------------------------------------------ context ----
int bamm_ctx_create(int device, void* hip_stream, bamm_ctx** out) {
    if (!out) { set_error("bamm_ctx_create: null out"); return BAMM_ERR_ARG; }
    *out = nullptr;
    if (int rc = check_device_index(device, device)) return rc;
    BAMM_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    BAMM_HIP(hipGetDeviceProperties(&prop, device));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0) {
        set_error("device %d is %s; this library only carries gfx950 code objects", device, prop.gcnArchName);
        return BAMM_ERR_NO_DEVICE;
    }
    bamm_ctx* c = new bamm_ctx();
    c->device = device;
    c->num_cus = prop.multiProcessorCount;
    c->name = prop.name;
    if (c->name.empty()) c->name = prop.gcnArchName;       // some driver stacks leave the marketing name blank
    if (hip_stream) {
        c->stream = (hipStream_t)hip_stream;
    } else {
        hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
        if (e != hipSuccess) {
            set_error("hipStreamCreate failed: %s", hipGetErrorString(e));
            delete c;
            return BAMM_ERR_HIP;
        }
        c->own_stream = true;
    }
    (void)prime_model_kernels();                             // k_make_s / k_update: the first kernels any handle launches
    {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) c->scratch_cap_bytes = total_b / 4;
        std::lock_guard<std::mutex> g(g_ctx_mu);
        g_ctxs.push_back(c);
    }
    *out = c;
    return BAMM_OK;
}

long long bamm_device_blocks_live(void) { return g_blocks_live.load(); }

int bamm_device_count(int* n) {
    if (!n) { set_error("bamm_device_count: null argument"); return BAMM_ERR_ARG; }
    *n = 0;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        set_error("no HIP device visible: the gfx950 extension cannot run (there is no CPU fallback)");
        return BAMM_ERR_NO_DEVICE;
    }
    *n = count;
    return BAMM_OK;
}

int bamm_device_pci_bus_id(int device, char* buf, size_t cap) {
    if (!buf || cap < 16) { set_error("bamm_device_pci_bus_id: buffer of at least 16 bytes"); return BAMM_ERR_ARG; }
    buf[0] = 0;
    if (int rc = check_device_index(device, device)) return rc;
    BAMM_HIP(hipDeviceGetPCIBusId(buf, (int)cap, device));
    return BAMM_OK;
}

int bamm_device_can_access_peer(int device, int peer, int* can) {
    if (!can) { set_error("bamm_device_can_access_peer: null argument"); return BAMM_ERR_ARG; }
    *can = 0;
    if (int rc = check_device_index(device, peer)) return rc;
    if (device == peer) { *can = 1; return BAMM_OK; }
    BAMM_HIP(hipDeviceCanAccessPeer(can, device, peer));
    return BAMM_OK;
}

int bamm_ctx_destroy(bamm_ctx* c) {
    if (!c) return BAMM_OK;
    {
        std::lock_guard<std::mutex> g(g_ctx_mu);
        g_ctxs.erase(std::remove(g_ctxs.begin(), g_ctxs.end(), c), g_ctxs.end());
    }
    (void)hipSetDevice(c->device);
    if (!c->scratch_idle.empty()) (void)hipStreamSynchronize(c->stream);
    for (auto& b : c->scratch_idle) (void)hipFree(b.first);
    if (c->stage_buf[0]) {
        (void)hipStreamSynchronize(c->stream);
        (void)hipHostFree(c->stage_buf[0]);
        for (hipEvent_t e : c->stage_ev) if (e) (void)hipEventDestroy(e);
    }
    if (c->own_stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return BAMM_OK;
}

int bamm_ctx_sync(bamm_ctx* c) {
    if (!c) { set_error("null ctx"); return BAMM_ERR_ARG; }
    BAMM_HIP(hipStreamSynchronize(c->stream));
    return BAMM_OK;
}

int bamm_ctx_device_name(bamm_ctx* c, char* buf, size_t cap) {
    if (!c || !buf || !cap) { set_error("bad argument"); return BAMM_ERR_ARG; }
    snprintf(buf, cap, "%s", c->name.c_str());
    return BAMM_OK;
}

int bamm_ctx_set_launch(bamm_ctx* c, uint32_t blocks, uint32_t threads) {
    if (!c || (threads & 63u) || threads > 1024u) { set_error("threads must be a multiple of 64 <= 1024"); return BAMM_ERR_ARG; }
    c->blocks = blocks;
    c->threads = threads;
    return BAMM_OK;
}

int bamm_ctx_set_tuning(bamm_ctx* c, const char* key, int value) {
    if (!c || !key) { set_error("bamm_ctx_set_tuning: null argument"); return BAMM_ERR_ARG; }
    for (const TuningKey& t : kTuningKeys) {
        if (strcmp(t.key, key) != 0) continue;
        if (t.range && (value < t.lo || value > t.hi) && value != t.also) { set_error("%s must be %s", key, t.range); return BAMM_ERR_ARG; }
        std::visit([c, value](auto field) {
            auto& f = c->*field;
            using T = std::remove_reference_t<decltype(f)>;
            if constexpr (std::is_same_v<T, bool>) f = value != 0;
            else if constexpr (std::is_same_v<T, size_t>) {       // scratch_cache_mb, in MiB
                f = (size_t)value << 20;
                if (value == 0) (void)flush_idle_scratch(c->device);
            } else f = (T)value;
        }, t.field);
        return BAMM_OK;
    }
    set_error("bamm_ctx_set_tuning: unknown key '%s'", key);
    return BAMM_ERR_ARG;
}

}  // extern "C"
