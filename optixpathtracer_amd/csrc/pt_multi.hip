// pt_multi: N contexts in one process (include/pt_amd.h), one enqueue thread per rank, strips exchanged over RCCL or peer copies.
// No reference counterpart: the reference is single-GPU.  Part of pt_lib.hip.
#include <dlfcn.h>
// declarations only: the pointer types below are RCCL's own, the library itself is opened at run time
#if __has_include(<rccl/rccl.h>)
#include <rccl/rccl.h>
#else // a box without RCCL's headers: the six prototypes as rccl.h (2.x) declares them, so that libptamd still builds (single-GPU path, peer copies)
typedef struct ncclComm* ncclComm_t;
typedef enum { ncclSuccess = 0 } ncclResult_t;
typedef enum { ncclInt8 = 0, ncclChar = 0, ncclUint8 = 1 } ncclDataType_t;
extern "C" {
ncclResult_t ncclCommInitAll(ncclComm_t* comm, int ndev, const int* devlist);
ncclResult_t ncclCommDestroy(ncclComm_t comm);
ncclResult_t ncclGroupStart();
ncclResult_t ncclGroupEnd();
ncclResult_t ncclAllGather(const void* sendbuff, void* recvbuff, size_t sendcount, ncclDataType_t datatype, ncclComm_t comm, hipStream_t stream);
const char* ncclGetErrorString(ncclResult_t result);
}
#endif

namespace {
// the six RCCL entry points the exchange needs, resolved at run time: libptamd must load (and the single-GPU path must
// work) on a box without librccl, and a process that already holds torch's bundled librccl must not get a second copy.
// The pointer types are decltype of rccl.h's declarations, so a signature change breaks the build instead of the call.
struct Rccl {
    void* lib = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    bool ok() const { return lib && CommInitAll && CommDestroy && GroupStart && GroupEnd && AllGather && GetErrorString; }
};
const ncclDataType_t kNcclUint8 = ncclUint8;

Rccl& rccl() {
    static Rccl r;
    static bool tried = false;
    if (!tried) {
        tried = true;
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            r.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (r.lib) break;
        }
        if (r.lib) {
            r.CommInitAll = (decltype(r.CommInitAll))dlsym(r.lib, "ncclCommInitAll");
            r.CommDestroy = (decltype(r.CommDestroy))dlsym(r.lib, "ncclCommDestroy");
            r.GroupStart = (decltype(r.GroupStart))dlsym(r.lib, "ncclGroupStart");
            r.GroupEnd = (decltype(r.GroupEnd))dlsym(r.lib, "ncclGroupEnd");
            r.AllGather = (decltype(r.AllGather))dlsym(r.lib, "ncclAllGather");
            r.GetErrorString = (decltype(r.GetErrorString))dlsym(r.lib, "ncclGetErrorString");
        }
    }
    return r;
}
thread_local std::string g_multi_error;
} // namespace

// One host thread per rank (pt_multi, an EnqueueWorker each): a frame is ~60 launches and events per device, so enqueueing the devices one
// after the other from one thread costs ndev x (60 x 5-8 us) — at a 1/8 share of a 1080p frame (1.3-1.8 ms of GPU work) more than the frame
// itself.  Every rank's thread enqueues its own device; the calling thread posts a job to each and waits for all.
struct pt_multi {
    std::vector<pt_ctx*> ctx;
    std::vector<int> devices;
    std::string err;
    bool distinct = true;           // no device appears twice (RCCL's requirement)
    std::vector<ncclComm_t> comms;  // per rank (empty until the first RCCL gather)
    int exchange_pref = 0;          // PT_MULTI_EXCHANGE: 0 auto, 1 rccl, 2 peer copies
    // The exchange strips of the current frame size: freed and rebuilt by pt_multi_resize.  send.empty(): not resized.
    struct Strips { std::vector<uint8_t*> send, recv; };
    struct Exchange {
        std::vector<DevOwner> mem;      // per rank: what the rank's device holds of the arrays and events below
        std::vector<uint8_t*> send, recv; // per rank: padded * 16 bytes, world * padded * 16 bytes (the synchronous pt_multi_gather)
        uint32_t padded = 0;
        Strips hand[2][6];              // the overlapped hand-off (below): [slot][pt_buffer], allocated on first use
        std::vector<hipEvent_t> xfer_done[2]; // peer-copy exchange: rank r's copies of slot s are complete
    } ex;
    double gather_ms = 0;
    int last_exchange = PT_EXCHANGE_NONE;
    std::vector<std::unique_ptr<EnqueueWorker>> workers; // empty: single rank or PT_MULTI_THREADS=0 (everything on the calling thread)
    double enqueue_ms = 0;          // host time of the enqueue phase of the last render: the slowest rank's
    // Overlapped hand-off (frames in flight + a gather mask): frame k's strips are packed behind frame k (pt_pack_async) into the
    // buffers of slot k & 1 and exchanged + scattered into the ranks' DISPLAY buffers by the NEXT render call, while frame k+1 renders.
    int pending_slot = -1;          // slot whose strips are packed (or being packed) but not yet exchanged
    uint32_t pending_mask = 0;
    uint64_t handed = 0;            // frames handed over through the overlapped path
    uint64_t packs = 0;             // pack rounds enqueued (slot = packs & 1)
};

static int mfail(pt_multi* m, int code, const std::string& msg) {
    if (m) m->err = msg; else g_multi_error = msg;
    return code;
}
// forward a per-context failure
static int mctx(pt_multi* m, int r, int rc, const char* what) {
    if (rc == PT_OK) return PT_OK;
    return mfail(m, rc, std::string(what) + " (rank " + std::to_string(r) + ", device " + std::to_string(m->devices[r]) + "): " + m->ctx[r]->err);
}
#define MCK(m, call)                                                                                  \
    do {                                                                                              \
        hipError_t e_ = (call);                                                                       \
        if (e_ != hipSuccess) return mfail(m, PT_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

extern "C" const char* pt_multi_last_error(const pt_multi* m) { return m ? m->err.c_str() : g_multi_error.c_str(); }
extern "C" int pt_multi_size(const pt_multi* m) { return m ? (int)m->ctx.size() : 0; }
extern "C" pt_ctx* pt_multi_ctx(pt_multi* m, int rank) { return (m && rank >= 0 && rank < (int)m->ctx.size()) ? m->ctx[rank] : nullptr; }

static int multi_present_pending(pt_multi* m, bool wait);
// the communicators: made by the first RCCL exchange
static int multi_comms(pt_multi* m) {
    if (!m->comms.empty()) return PT_OK;
    m->comms.assign(m->ctx.size(), nullptr);
    const ncclResult_t e = rccl().CommInitAll(m->comms.data(), (int)m->ctx.size(), m->devices.data());
    if (e == ncclSuccess) return PT_OK;
    m->comms.clear();
    return mfail(m, PT_ERR_HIP, std::string("ncclCommInitAll: ") + rccl().GetErrorString(e));
}
static void multi_unset_exchange(pt_multi* m) {
    for (size_t r = 0; r < m->ctx.size(); ++r) { // pending packs / exchanges run on the contexts' streams
        hipSetDevice(m->devices[r]);
        if (m->ctx[r] && m->ctx[r]->stream) hipStreamSynchronize(m->ctx[r]->stream);
    }
    for (size_t r = 0; r < m->ex.mem.size(); ++r) {
        hipSetDevice(m->devices[r]);
        m->ex.mem[r].release();
    }
    m->ex = pt_multi::Exchange{};
    m->pending_slot = -1;
    m->pending_mask = 0;
}

// fn(rank) for every rank, concurrently on the ranks' threads (or one after the other on the calling thread); returns the first
// failing rank's status, forwarded with its message.  max_ms: host time of the slowest rank.
static int multi_run(pt_multi* m, const std::function<int(int)>& fn, const char* what, double* max_ms = nullptr) {
    const int world = (int)m->ctx.size();
    std::vector<int> rcs(world, PT_OK);
    double slow = 0;
    if (m->workers.empty()) {
        for (int r = 0; r < world; ++r) {
            const auto t0 = std::chrono::steady_clock::now();
            rcs[r] = fn(r);
            slow += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); // serial: the times add up
        }
    } else {
        for (int r = 0; r < world; ++r) enqueue_worker_post(m->workers[r].get(), [&fn, r] { return fn(r); });
        for (int r = 0; r < world; ++r) {
            rcs[r] = enqueue_worker_wait(m->workers[r].get());
            slow = std::max(slow, m->workers[r]->ms); // (written before `done`, which the wait has seen)
        }
    }
    if (max_ms) *max_ms = slow;
    for (int r = 0; r < world; ++r)
        if (rcs[r] != PT_OK) return mctx(m, r, rcs[r], what);
    return PT_OK;
}

extern "C" int pt_multi_destroy(pt_multi* m) {
    if (!m) return PT_OK;
    for (auto& w : m->workers) enqueue_worker_stop(w.get());
    m->workers.clear();
    multi_unset_exchange(m);
    if (!m->comms.empty() && rccl().ok())
        for (ncclComm_t c : m->comms)
            if (c) rccl().CommDestroy(c);
    for (pt_ctx* c : m->ctx) pt_destroy(c);
    delete m;
    return PT_OK;
}

extern "C" int pt_create_multi(const pt_scene_desc* scene, const int* devices, int ndev, pt_multi** out) {
    if (!out || !devices || ndev < 1 || ndev > 64) return mfail(nullptr, PT_ERR_INVALID, "pt_create_multi: need 1..64 devices and an output pointer");
    FlatScene fs; // ONE host-side flatten + validation, shared by all ranks
    int rc = flatten_scene(scene, fs);
    if (rc != PT_OK) return mfail(nullptr, rc, g_create_error);
    pt_multi* m = new pt_multi();
    m->devices.assign(devices, devices + ndev);
    for (int a = 0; a < ndev; ++a)
        for (int b = a + 1; b < ndev; ++b)
            if (devices[a] == devices[b]) m->distinct = false;
    if (const char* e = getenv("PT_MULTI_EXCHANGE")) m->exchange_pref = !strcmp(e, "rccl") ? 1 : (!strcmp(e, "peer") ? 2 : 0);
    for (int r = 0; r < ndev; ++r) {
        pt_ctx* c = nullptr;
        rc = create_from_flat(fs, devices[r], &c);
        if (rc != PT_OK) {
            const std::string msg = "pt_create_multi: rank " + std::to_string(r) + ": " + g_create_error;
            pt_multi_destroy(m);
            return mfail(nullptr, rc, msg);
        }
        m->ctx.push_back(c);
    }
    // direct device-to-device copies between distinct devices need peer access (xGMI); failure is not fatal — hipMemcpyPeerAsync
    // then stages through the host
    if (m->distinct && ndev > 1)
        for (int a = 0; a < ndev; ++a) {
            hipSetDevice(devices[a]);
            for (int b = 0; b < ndev; ++b) {
                int can = 0;
                if (a != b && hipDeviceCanAccessPeer(&can, devices[a], devices[b]) == hipSuccess && can) {
                    hipError_t e = hipDeviceEnablePeerAccess(devices[b], 0);
                    if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
                }
            }
        }
    const char* te = getenv("PT_MULTI_THREADS");
    if (ndev > 1 && !(te && atoi(te) == 0))
        for (int r = 0; r < ndev; ++r) {
            m->workers.emplace_back(new EnqueueWorker());
            m->workers.back()->th = std::thread(enqueue_worker_main, m->workers.back().get(), devices[r]);
        }
    *out = m;
    return PT_OK;
}

// one setter on every rank, in rank order: the first failing rank's status goes out through mctx
template <class Call>
static int multi_each(pt_multi* m, const char* what, Call call) {
    for (size_t r = 0; r < m->ctx.size(); ++r) {
        int rc = mctx(m, (int)r, call(m->ctx[r]), what);
        if (rc) return rc;
    }
    return PT_OK;
}
extern "C" int pt_multi_set_options(pt_multi* m, const pt_options* opt) {
    if (!m || !opt) return PT_ERR_INVALID;
    return multi_each(m, "pt_multi_set_options", [&](pt_ctx* c) { return pt_set_options(c, opt); });
}
extern "C" int pt_multi_set_probe(pt_multi* m, const float* data, const float* pdfX, const float* cdfX, const float* pdfY, const float* cdfY, int w, int h) {
    if (!m) return PT_ERR_INVALID;
    return multi_each(m, "pt_multi_set_probe", [&](pt_ctx* c) { return pt_set_probe(c, data, pdfX, cdfX, pdfY, cdfY, w, h); });
}
extern "C" int pt_multi_set_probe_image(pt_multi* m, const float* data, int w, int h) {
    if (!m) return PT_ERR_INVALID;
    return multi_each(m, "pt_multi_set_probe_image", [&](pt_ctx* c) { return pt_set_probe_image(c, data, w, h); });
}
extern "C" int pt_multi_set_camera(pt_multi* m, const float eye[3], const float U[3], const float V[3], const float W[3]) {
    if (!m) return PT_ERR_INVALID;
    return multi_each(m, "pt_multi_set_camera", [&](pt_ctx* c) { return pt_set_camera(c, eye, U, V, W); });
}

extern "C" int pt_multi_set_views(pt_multi* m, const pt_view* views, uint32_t n) {
    if (!m) return PT_ERR_INVALID;
    return multi_each(m, "pt_multi_set_views", [&](pt_ctx* c) { return pt_set_views(c, views, n); });
}
extern "C" int pt_multi_set_view_cameras(pt_multi* m, const float* cams, uint32_t n) {
    if (!m) return PT_ERR_INVALID;
    return multi_each(m, "pt_multi_set_view_cameras", [&](pt_ctx* c) { return pt_set_view_cameras(c, cams, n); });
}

extern "C" int pt_multi_resize(pt_multi* m, int width, int height, int tile_w, int tile_h) {
    if (!m) return PT_ERR_INVALID;
    if (width == 0 || height == 0) return PT_OK;
    if (tile_w == 0) tile_w = 64;
    if (tile_h == 0) tile_h = 16;
    const int world = (int)m->ctx.size();
    multi_unset_exchange(m);
    std::vector<uint8_t*> send(world, nullptr), recv(world, nullptr);
    m->ex.mem.resize(world);
    auto build = [&]() -> int {
        for (int r = 0; r < world; ++r) {
            pt_ctx* c = m->ctx[r];
            c->width = c->height = 0; // pt_set_partition then only records the partition; pt_resize applies it
            int rc = mctx(m, r, pt_set_partition(c, r, world, tile_w, tile_h), "pt_multi_resize");
            if (rc == PT_OK) rc = mctx(m, r, pt_resize(c, width, height), "pt_multi_resize");
            if (rc) return rc;
        }
        const size_t padded = m->ctx[0]->padded;
        for (int r = 0; r < world; ++r) {
            MCK(m, hipSetDevice(m->devices[r]));
            MCK(m, m->ex.mem[r].alloc(&send[r], std::max<size_t>(16, padded * 16)));
            MCK(m, m->ex.mem[r].alloc(&recv[r], std::max<size_t>(16, (size_t)world * padded * 16)));
        }
        return PT_OK;
    };
    const int rc = build();
    if (rc) { // every rank is as before its first resize: none keeps a frame that the others, or the strips, lack
        for (pt_ctx* c : m->ctx) drain(c); // (a rank the loop did not reach may have frames in flight)
        multi_unset_exchange(m);           // (waits for the ranks' streams)
        for (int r = 0; r < world; ++r) {
            hipSetDevice(m->devices[r]);
            unset_frame(m->ctx[r]);
        }
        return rc;
    }
    m->ex.padded = m->ctx[0]->padded;
    m->ex.send = send;
    m->ex.recv = recv;
    return PT_OK;
}

extern "C" int pt_multi_gather(pt_multi* m, int which) {
    if (!m) return PT_ERR_INVALID;
    const int world = (int)m->ctx.size();
    if (m->ex.send.empty()) return mfail(m, PT_ERR_INVALID, "pt_multi_gather: not resized");
    size_t elem = 0;
    if (!buffer_ptr(m->ctx[0], which, &elem)) return mfail(m, PT_ERR_INVALID, "pt_multi_gather: unknown buffer");
    const size_t bytes = (size_t)m->ex.padded * elem; // one rank's packed strip (padded to the largest share: same on every rank)
    {
        int rc = multi_present_pending(m, true); // a frame of the overlapped path that was still waiting for its hand-over
        if (rc) return rc;
    }
    for (int r = 0; r < world; ++r) { // frames in flight (pt_options.frames_in_flight) are not ordered before the contexts' own streams
        int rc = mctx(m, r, drain(m->ctx[r]), "pt_multi_gather");
        if (rc) return rc;
    }
    const auto t0 = std::chrono::steady_clock::now();
    for (int r = 0; r < world; ++r) {
        int rc = mctx(m, r, pack_launch(m->ctx[r], which, m->ex.send[r]), "pt_multi_gather(pack)");
        if (rc) return rc;
    }
    DevOwner tmp; // the peer copies' events: they must outlive the waits, so they go when the streams have been synchronised, below
    bool use_rccl = m->exchange_pref == 1 || (m->exchange_pref == 0 && m->distinct && world > 1);
    if (use_rccl && (!rccl().ok() || !m->distinct)) {
        if (m->exchange_pref == 1) return mfail(m, PT_ERR_UNSUPPORTED, !m->distinct ? "pt_multi_gather: RCCL needs distinct devices" : "pt_multi_gather: librccl not found");
        use_rccl = false;
    }
    if (use_rccl) {
        Rccl& R = rccl();
        if (int rc = multi_comms(m)) return rc;
        // one all-gather of `bytes` per rank: with 8 GPUs each of the 7 xGMI links of a GPU carries one strip
        ncclResult_t e = R.GroupStart();
        for (int r = 0; r < world && e == ncclSuccess; ++r) {
            MCK(m, hipSetDevice(m->devices[r]));
            e = R.AllGather(m->ex.send[r], m->ex.recv[r], bytes, kNcclUint8, m->comms[r], m->ctx[r]->stream);
        }
        const ncclResult_t e2 = R.GroupEnd();
        if (e != ncclSuccess || e2 != ncclSuccess) return mfail(m, PT_ERR_HIP, std::string("ncclAllGather: ") + R.GetErrorString(e != ncclSuccess ? e : e2));
        m->last_exchange = PT_EXCHANGE_RCCL;
    } else {
        // every rank writes its strip into slot r of every rank's receive buffer (direct peer writes over xGMI; a plain
        // device-to-device copy when both ranks live on one device), then every rank waits for all writers
        std::vector<hipEvent_t> done(world);
        for (int r = 0; r < world; ++r) {
            MCK(m, hipSetDevice(m->devices[r]));
            for (int p = 0; p < world; ++p) {
                char* dst = (char*)m->ex.recv[p] + (size_t)r * bytes;
                if (m->devices[p] == m->devices[r]) MCK(m, hipMemcpyAsync(dst, m->ex.send[r], bytes, hipMemcpyDeviceToDevice, m->ctx[r]->stream));
                else MCK(m, hipMemcpyPeerAsync(dst, m->devices[p], m->ex.send[r], m->devices[r], bytes, m->ctx[r]->stream));
            }
            MCK(m, tmp.event(&done[r], hipEventDisableTiming));
            MCK(m, hipEventRecord(done[r], m->ctx[r]->stream));
        }
        for (int p = 0; p < world; ++p) {
            MCK(m, hipSetDevice(m->devices[p]));
            for (int r = 0; r < world; ++r)
                if (r != p) MCK(m, hipStreamWaitEvent(m->ctx[p]->stream, done[r], 0));
        }
        m->last_exchange = PT_EXCHANGE_PEER_COPY;
    }
    for (int r = 0; r < world; ++r) {
        int rc = mctx(m, r, unpack_launch(m->ctx[r], which, m->ex.recv[r]), "pt_multi_gather(unpack)");
        if (rc) return rc;
    }
    for (int r = 0; r < world; ++r) {
        MCK(m, hipSetDevice(m->devices[r]));
        MCK(m, hipStreamSynchronize(m->ctx[r]->stream));
    }
    m->gather_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return PT_OK;
}

static int multi_after_render(pt_multi* m, uint32_t gather_mask, uint32_t* host_rgba8) {
    if (host_rgba8) gather_mask |= 1u << PT_BUF_FRAME;
    if (m->ctx[0]->width == 0) return PT_OK;
    for (int which = 0; which <= PT_BUF_DENOISED; ++which)
        if (gather_mask & (1u << which)) {
            int rc = pt_multi_gather(m, which);
            if (rc) return rc;
        }
    if (host_rgba8) return mctx(m, 0, pt_download(m->ctx[0], PT_BUF_FRAME, host_rgba8, sizeof(uint32_t) * (size_t)m->ctx[0]->width * m->ctx[0]->height), "pt_multi_render(download)");
    return PT_OK;
}

// ---- overlapped hand-off (frames in flight + something to hand over): everything below only ENQUEUES on the ranks' own streams
static int multi_ensure_strips(pt_multi* m, int slot, int which) {
    pt_multi::Exchange& X = m->ex;
    pt_multi::Strips& st = X.hand[slot][which];
    const int world = (int)m->ctx.size();
    if (X.send.empty()) return mfail(m, PT_ERR_INVALID, "pt_multi: not resized"); // X.padded sizes the strips
    if ((int)st.send.size() == world) return PT_OK;
    const size_t elem = buffer_elem(which);
    // built aside and published whole: strips that are half there would pass for complete
    std::vector<uint8_t*> send(world, nullptr), recv(world, nullptr);
    std::vector<hipEvent_t> done(X.xfer_done[slot].empty() ? world : 0, nullptr);
    auto build = [&]() -> int {
        for (int r = 0; r < world; ++r) {
            MCK(m, hipSetDevice(m->devices[r]));
            MCK(m, X.mem[r].alloc(&send[r], std::max<size_t>(16, (size_t)X.padded * elem)));
            MCK(m, X.mem[r].alloc(&recv[r], std::max<size_t>(16, (size_t)world * X.padded * elem)));
        }
        for (size_t r = 0; r < done.size(); ++r) {
            MCK(m, hipSetDevice(m->devices[r]));
            MCK(m, X.mem[r].event(&done[r], hipEventDisableTiming));
        }
        return PT_OK;
    };
    const int rc = build();
    if (rc) {
        for (int r = 0; r < world; ++r) {
            hipSetDevice(m->devices[r]);
            X.mem[r].drop(send[r]);
            X.mem[r].drop(recv[r]);
            if (!done.empty()) X.mem[r].drop(done[r]);
        }
        return rc;
    }
    st.send = send;
    st.recv = recv;
    if (!done.empty()) X.xfer_done[slot] = done;
    return PT_OK;
}
static bool multi_use_rccl(pt_multi* m, int* err) {
    const int world = (int)m->ctx.size();
    bool use_rccl = m->exchange_pref == 1 || (m->exchange_pref == 0 && m->distinct && world > 1);
    *err = PT_OK;
    if (use_rccl && (!rccl().ok() || !m->distinct)) {
        if (m->exchange_pref == 1) *err = mfail(m, PT_ERR_UNSUPPORTED, !m->distinct ? "pt_multi: RCCL needs distinct devices" : "pt_multi: librccl not found");
        use_rccl = false;
    }
    return use_rccl;
}
// the strips of `slot` (packed on every rank's stream) -> all ranks' receive buffers -> the ranks' display buffers
static int multi_exchange_display(pt_multi* m, int slot, int which) {
    const int world = (int)m->ctx.size();
    pt_multi::Strips& st = m->ex.hand[slot][which];
    const size_t bytes = (size_t)m->ex.padded * buffer_elem(which);
    int err;
    const bool use_rccl = multi_use_rccl(m, &err);
    if (err) return err;
    if (use_rccl) {
        Rccl& R = rccl();
        if (int rc = multi_comms(m)) return rc;
        ncclResult_t e = R.GroupStart();
        for (int r = 0; r < world && e == ncclSuccess; ++r) {
            MCK(m, hipSetDevice(m->devices[r]));
            e = R.AllGather(st.send[r], st.recv[r], bytes, kNcclUint8, m->comms[r], m->ctx[r]->stream);
        }
        const ncclResult_t e2 = R.GroupEnd();
        if (e != ncclSuccess || e2 != ncclSuccess) return mfail(m, PT_ERR_HIP, std::string("ncclAllGather: ") + R.GetErrorString(e != ncclSuccess ? e : e2));
        m->last_exchange = PT_EXCHANGE_RCCL;
    } else {
        for (int r = 0; r < world; ++r) {
            MCK(m, hipSetDevice(m->devices[r]));
            for (int p = 0; p < world; ++p) {
                char* dst = (char*)st.recv[p] + (size_t)r * bytes;
                if (m->devices[p] == m->devices[r]) MCK(m, hipMemcpyAsync(dst, st.send[r], bytes, hipMemcpyDeviceToDevice, m->ctx[r]->stream));
                else MCK(m, hipMemcpyPeerAsync(dst, m->devices[p], st.send[r], m->devices[r], bytes, m->ctx[r]->stream));
            }
            MCK(m, hipEventRecord(m->ex.xfer_done[slot][r], m->ctx[r]->stream));
        }
        for (int p = 0; p < world; ++p) {
            MCK(m, hipSetDevice(m->devices[p]));
            for (int r = 0; r < world; ++r)
                if (r != p) MCK(m, hipStreamWaitEvent(m->ctx[p]->stream, m->ex.xfer_done[slot][r], 0));
        }
        m->last_exchange = PT_EXCHANGE_PEER_COPY;
    }
    for (int r = 0; r < world; ++r) {
        int rc = mctx(m, r, unpack_display_enqueue(m->ctx[r], which, st.recv[r]), "pt_multi(unpack_display)");
        if (rc) return rc;
    }
    return PT_OK;
}
// exchange what the previous call packed (if anything) and wait until it is on display
static int multi_present_pending(pt_multi* m, bool wait) {
    if (m->pending_slot < 0) return PT_OK;
    const int slot = m->pending_slot;
    const uint32_t mask = m->pending_mask;
    m->pending_slot = -1;
    m->pending_mask = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (int which = 0; which <= PT_BUF_DENOISED; ++which)
        if (mask & (1u << which)) {
            int rc = multi_exchange_display(m, slot, which);
            if (rc) return rc;
        }
    ++m->handed;
    if (wait)
        for (size_t r = 0; r < m->ctx.size(); ++r) {
            int rc = mctx(m, (int)r, pt_display_sync(m->ctx[r]), "pt_multi(display)");
            if (rc) return rc;
        }
    m->gather_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return PT_OK;
}
static int multi_pack_newest(pt_multi* m, uint32_t mask) {
    // the slots alternate: the other slot's strips were exchanged by this call a moment ago (they may still be in flight), this slot's
    // were put on display — and waited for — one call earlier
    const int use = (int)(m->packs++ & 1);
    for (int which = 0; which <= PT_BUF_DENOISED; ++which)
        if (mask & (1u << which)) {
            int rc = multi_ensure_strips(m, use, which);
            if (rc) return rc;
            for (size_t r = 0; r < m->ctx.size(); ++r) {
                rc = mctx(m, (int)r, pack_async_enqueue(m->ctx[r], which, m->ex.hand[use][which].send[r], use), "pt_multi(pack)");
                if (rc) return rc;
            }
        }
    m->pending_slot = use;
    m->pending_mask = mask;
    return PT_OK;
}

// One frame (or launch chain of `count` subframes, or — regions != null — one foveated frame) on every rank.
static int multi_render_common(pt_multi* m, uint32_t spp, uint32_t subframe_index, uint32_t count, const pt_region* regions, uint32_t nreg,
                               const pt_variant* variant, uint32_t gather_mask, uint32_t* host_rgba8, const char* what) {
    const int world = (int)m->ctx.size();
    if (world == 0) return PT_OK;
    if (host_rgba8) gather_mask |= 1u << PT_BUF_FRAME;
    if (gather_mask >> (PT_BUF_DENOISED + 1)) return mfail(m, PT_ERR_INVALID, std::string(what) + ": unknown buffer in gather_mask");
    const int F = frames_mode(m->ctx[0]);
    auto enqueue = [&](int r, int slot, int mode) {
        pt_ctx* c = m->ctx[r];
        return regions ? regions_enqueue(c, regions, nreg, variant, slot, mode != 0) : render_enqueue(c, spp, subframe_index, slot, mode, count);
    };
    auto enqueue_pipelined = [&](int r) { return enqueue_next_slot(m->ctx[r], F, [&](int slot) { return enqueue(r, slot, F); }); };
    if (F > 1 && gather_mask == 0) {
        // pure throughput (nothing is handed over after this frame): pt_options.frames_in_flight applies on every device
        int rc = multi_present_pending(m, true); // a frame of an earlier call that was waiting for its hand-over
        int rc1 = multi_run(m, enqueue_pipelined, what, &m->enqueue_ms);
        int rc2 = multi_run(m, [&](int r) { return pipelined_wait(m->ctx[r], F); }, what);
        return rc ? rc : (rc1 ? rc1 : rc2);
    }
    if (F > 1) {
        // Frames in flight AND a hand-over: frame k is enqueued, then the strips frame k-1 packed behind itself are exchanged and
        // scattered into the display buffers while frame k renders, then frame k's pack is enqueued behind frame k.  The call
        // returns when frame k-1 is on display (host_rgba8 receives it) and at most F-1 frames are still running.
        int rc = multi_run(m, enqueue_pipelined, what, &m->enqueue_ms);
        if (rc) return rc;
        const bool had = m->pending_slot >= 0;
        rc = multi_present_pending(m, true);
        if (rc) return rc;
        if (m->ctx[0]->width) {
            rc = multi_pack_newest(m, gather_mask);
            if (rc) return rc;
        }
        rc = multi_run(m, [&](int r) { return pipelined_wait(m->ctx[r], F); }, what);
        if (rc) return rc;
        if (host_rgba8 && had && m->ctx[0]->width)
            return mctx(m, 0, pt_download_display(m->ctx[0], PT_BUF_FRAME, host_rgba8, sizeof(uint32_t) * (size_t)m->ctx[0]->width * m->ctx[0]->height), what);
        return PT_OK;
    }
    // synchronous frames: every rank enqueues and finishes its own frame on its own thread, then the hand-over
    int rc = multi_present_pending(m, true);
    if (rc) return rc;
    rc = multi_run(m, [&](int r) { return enqueue(r, 0, 0); }, what, &m->enqueue_ms);
    int rc2 = multi_run(m, [&](int r) { return render_finish(m->ctx[r]); }, what); // every rank's frame is waited for, also after a failure
    if (rc || rc2) return rc ? rc : rc2;
    return multi_after_render(m, gather_mask, host_rgba8);
}

extern "C" int pt_multi_render(pt_multi* m, uint32_t spp, uint32_t subframe_index, uint32_t gather_mask, uint32_t* host_rgba8) {
    return pt_multi_render_batch(m, spp, subframe_index, 1, gather_mask, host_rgba8);
}

extern "C" int pt_multi_render_batch(pt_multi* m, uint32_t spp, uint32_t subframe_index, uint32_t count, uint32_t gather_mask, uint32_t* host_rgba8) {
    if (!m) return PT_ERR_INVALID;
    return multi_render_common(m, spp, subframe_index, count, nullptr, 0, nullptr, gather_mask, host_rgba8, "pt_multi_render");
}

extern "C" int pt_multi_render_regions(pt_multi* m, const pt_region* regions, uint32_t n, const pt_variant* variant, uint32_t gather_mask, uint32_t* host_rgba8) {
    if (!m || (!regions && n)) return PT_ERR_INVALID;
    if (!m->ctx.empty() && m->ctx[0]->vw.n) return mfail(m, PT_ERR_UNSUPPORTED, "pt_multi_render_regions: not with viewports set (pt_multi_set_views)");
    return multi_render_common(m, 0, 0, 1, regions, n, variant, gather_mask, host_rgba8, "pt_multi_render_regions");
}

// the frame that is still waiting for its hand-over (overlapped path) is exchanged and put on display
extern "C" int pt_multi_flush(pt_multi* m, uint32_t* host_rgba8) {
    if (!m) return PT_ERR_INVALID;
    const bool had = m->pending_slot >= 0;
    const bool frame = had && (m->pending_mask & (1u << PT_BUF_FRAME));
    int rc = multi_present_pending(m, true);
    if (rc) return rc;
    if (host_rgba8 && frame && !m->ctx.empty() && m->ctx[0]->width)
        return mctx(m, 0, pt_download_display(m->ctx[0], PT_BUF_FRAME, host_rgba8, sizeof(uint32_t) * (size_t)m->ctx[0]->width * m->ctx[0]->height), "pt_multi_flush");
    return PT_OK;
}

extern "C" int pt_multi_get_stats(const pt_multi* m, pt_multi_stats* out) {
    if (!m || !out) return PT_ERR_INVALID;
    memset(out, 0, sizeof(*out));
    for (size_t r = 0; r < m->ctx.size(); ++r) {
        pt_stats s;
        pt_get_stats(m->ctx[r], &s);
        out->sum.radiance_rays += s.radiance_rays;
        out->sum.shadow_rays += s.shadow_rays;
        out->sum.shaded_hits += s.shaded_hits;
        out->sum.paths += s.paths;
        out->sum.frames += s.frames; // frames x ranks
        out->sum.total_radiance_rays += s.total_radiance_rays;
        out->sum.total_shadow_rays += s.total_shadow_rays;
        out->sum.render_ms = std::max(out->sum.render_ms, s.render_ms);
        out->sum.trace_ms = std::max(out->sum.trace_ms, s.trace_ms);
        out->sum.shadow_ms = std::max(out->sum.shadow_ms, s.shadow_ms);
        out->sum.shade_ms = std::max(out->sum.shade_ms, s.shade_ms);
        out->sum.other_ms = std::max(out->sum.other_ms, s.other_ms);
        out->sum.trace_launches += s.trace_launches;
        out->sum.shadow_launches += s.shadow_launches;
        out->sum.shade_launches += s.shade_launches;
        out->sum.fused_passes += s.fused_passes;
        out->sum.bvh_nodes = s.bvh_nodes;
        out->sum.bvh_bytes = s.bvh_bytes;
        out->sum.bvh_levels = s.bvh_levels;
        out->sum.bvh_builder = s.bvh_builder;
        out->sum.bvh_build_ms = std::max(out->sum.bvh_build_ms, s.bvh_build_ms);
    }
    out->gather_ms = m->gather_ms;
    out->exchange = m->last_exchange;
    out->ndev = (int)m->ctx.size();
    out->enqueue_ms = m->enqueue_ms;
    out->threads = (int32_t)m->workers.size();
    out->frames_handed_over = m->handed;
    return PT_OK;
}

// stage on every rank, then commit on every rank: an update that one rank refuses changes none
static int multi_update(pt_multi* m, const UpdateSource& S, int mode, double* kernel_ms, const char* what) {
    const int world = (int)m->ctx.size();
    int rc = PT_OK;
    std::vector<MeshUpdate> U(world);
    for (int r = 0; r < world && rc == PT_OK; ++r) rc = mctx(m, r, update_stage(m->ctx[r], S, mode, U[r]), what);
    double slow = 0;
    for (int r = 0; r < world && rc == PT_OK; ++r) {
        double ms = 0;
        rc = mctx(m, r, update_commit(m->ctx[r], mode, U[r], &ms), what);
        slow = std::max(slow, ms);
    }
    if (rc == PT_OK && kernel_ms) *kernel_ms = slow;
    return rc;
}
extern "C" int pt_multi_update_meshes(pt_multi* m, const pt_mesh_update* updates, uint32_t n, int mode, double* kernel_ms) {
    if (!m) return PT_ERR_INVALID;
    std::string err;
    const int rc = update_validate(m->ctx[0], updates, n, mode, err);
    if (rc != PT_OK) return mfail(m, rc, err);
    UpdateSource S{"pt_update_meshes"};
    S.host = updates;
    S.n = n;
    return multi_update(m, S, mode, kernel_ms, "pt_multi_update_meshes");
}

extern "C" int pt_multi_transform_meshes(pt_multi* m, const pt_mesh_transform* t, uint32_t n, int source, int mode, double* kernel_ms) {
    if (!m) { (void)fail(nullptr, PT_ERR_INVALID, "pt_multi_transform_meshes: null pt_multi"); return mfail(nullptr, PT_ERR_INVALID, "pt_multi_transform_meshes: null pt_multi"); }
    std::string err;
    const int rc = transform_validate(m->ctx[0], t, n, source, mode, err, "pt_multi_transform_meshes");
    if (rc != PT_OK) return mfail(m, rc, err);
    UpdateSource S{"pt_multi_transform_meshes"};
    S.xform = t;
    S.from = source;
    S.n = n;
    return multi_update(m, S, mode, kernel_ms, "pt_multi_transform_meshes");
}
