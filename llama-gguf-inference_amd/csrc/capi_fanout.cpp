// capi_fanout.cpp — the replica fan-out over RCCL (include/llmi.h: llmi_replicate,
// llmi_model_load_replicated, llmi_model_fanout, llmi_model_load_fanout) and the arena
// hashes its verification rests on.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/llmi.h"
#include "capi_internal.h"

using namespace llmi;

extern "C" {

int32_t llmi_model_arena(const struct llama_model* model, void** dev_ptr, uint64_t* bytes) {
    if (!model) return -1;
    if (dev_ptr) *dev_ptr = model->m.arena;
    if (bytes) *bytes = model->m.arena_bytes;
    return 0;
}

// synchronous hash of device memory on `device` (launch_arena_hash, kernels.hip)
static bool device_hash(int device, const void* p, size_t bytes, uint64_t* out, std::string& err) {
    if (hipSetDevice(device) != hipSuccess) { err = "hipSetDevice"; return false; }
    DevPool P;
    unsigned long long* d = nullptr;
    if (P.alloc(d, 8) != hipSuccess) { err = "hipMalloc (hash)"; return false; }
    hipError_t e = launch_arena_hash(p, bytes, d, nullptr);
    if (e == hipSuccess) e = hipMemcpy(out, d, 8, hipMemcpyDeviceToHost);
    if (e != hipSuccess) { err = std::string("arena hash: ") + hipGetErrorString(e); return false; }
    return true;
}

int32_t llmi_model_arena_hash(const struct llama_model* model, uint64_t* out) {
    API_TRY
    if (!model || !out || !model->m.arena) { set_err("llmi_model_arena_hash: bad arguments"); return -1; }
    std::string err;
    if (!device_hash(model->m.device, model->m.arena, model->m.arena_bytes, out, err)) { set_err(err); return -2; }
    return 0;
    API_CATCH(-5)
}

int32_t llmi_device_hash(const void* dev_ptr, uint64_t bytes, uint64_t* out) {
    API_TRY
    if (!dev_ptr || !out) { set_err("llmi_device_hash: bad arguments"); return -1; }
    hipPointerAttribute_t at{};
    int dev = 0;
    if (hipPointerGetAttributes(&at, dev_ptr) == hipSuccess && at.device >= 0) dev = at.device;
    else (void)hipGetDevice(&dev);
    std::string err;
    if (!device_hash(dev, dev_ptr, (size_t)bytes, out, err)) { set_err(err); return -2; }
    return 0;
    API_CATCH(-5)
}

// ---- replica fan-out ------------------------------------------------
// The arena goes out in kFanoutChunk (256 MB) pieces on real streams.  When the source is
// still uploading (llmi_model_load_fanout / llmi_model_load_replicated), piece k is issued
// as soon as the upload stream has completed the arena prefix that covers it (an event on
// the upload stream, waited on by the broadcast streams), so the xGMI broadcast runs
// behind the host-to-device copy instead of after it.  model.cpp fanout_plan states the
// schedule; tests/test_fanout_plan.py checks it.
namespace {
struct Fanout {
    // one rank per entry: (device, arena, comm, stream); entry 0 is the root
    std::vector<int> dev;
    std::vector<uint8_t*> buf;
    std::vector<ncclComm_t> comm;
    std::vector<hipStream_t> st;
    size_t bytes = 0, next = 0;  // arena bytes; first piece not yet issued
    std::vector<hipEvent_t> evs;
    bool ok = true;        // every step so far succeeded
    bool nccl_ok = true;   // no ncclBroadcast failed: pieces must still be issued (the other
                           // ranks wait in their matching broadcasts), whatever else failed

    ~Fanout() {
        for (size_t r = 0; r < st.size(); ++r) {
            (void)hipSetDevice(dev[r]);
            if (st[r]) (void)hipStreamSynchronize(st[r]);
        }
        for (size_t r = 0; r < comm.size(); ++r)
            if (comm[r]) ncclCommDestroy(comm[r]);
        for (size_t r = 0; r < st.size(); ++r) {
            (void)hipSetDevice(dev[r]);
            if (st[r]) (void)hipStreamDestroy(st[r]);
        }
        for (hipEvent_t e : evs) (void)hipEventDestroy(e);
    }
    bool make_streams() {
        st.assign(dev.size(), nullptr);
        for (size_t r = 0; r < dev.size(); ++r) {
            if (hipSetDevice(dev[r]) != hipSuccess) return false;
            if (hipStreamCreateWithFlags(&st[r], hipStreamNonBlocking) != hipSuccess) return false;
        }
        return true;
    }
    // issue every piece that ends at or before `prefix` (all of them if prefix >= bytes);
    // `wait`: an event on the root's upload stream the broadcast streams wait on first
    bool issue(size_t prefix, hipEvent_t wait) {
        bool waited = false;
        while (nccl_ok && next * kFanoutChunk < bytes) {
            const size_t off = next * kFanoutChunk, len = std::min(kFanoutChunk, bytes - off);
            if (off + len > prefix) break;
            if (wait && !waited) {
                for (size_t r = 0; r < dev.size(); ++r) {
                    (void)hipSetDevice(dev[r]);
                    if (hipStreamWaitEvent(st[r], wait, 0) != hipSuccess) {
                        ok = false;  // the piece still goes out, after the upload reached it
                        (void)hipEventSynchronize(wait);
                    }
                }
                waited = true;
            }
            ncclResult_t nr = dev.size() > 1 ? ncclGroupStart() : ncclSuccess;
            for (size_t r = 0; r < dev.size() && nr == ncclSuccess; ++r) {
                (void)hipSetDevice(dev[r]);
                nr = ncclBroadcast(buf[r] + off, buf[r] + off, len, ncclUint8, 0, comm[r], st[r]);
            }
            if (dev.size() > 1) {
                const ncclResult_t ne = ncclGroupEnd();
                if (nr == ncclSuccess) nr = ne;
            }
            if (nr != ncclSuccess) ok = nccl_ok = false;
            ++next;
        }
        return ok;
    }
    bool finish() {
        issue(bytes, nullptr);
        for (size_t r = 0; r < dev.size(); ++r) {
            (void)hipSetDevice(dev[r]);
            if (hipStreamSynchronize(st[r]) != hipSuccess) ok = false;
        }
        return ok;
    }
    // After finish(): the root's {status, arena hash} goes to every rank of the
    // communicator (one more broadcast, so every rank leaves the fan-out together), and
    // each rank compares its own arena's hash with the root's.  root_ok: the caller's own
    // view of the root's load (upload + pieces).  Returns whether THIS process's ranks
    // hold the root's bytes; err says why not.  (a rank used to return
    // success with a partly written arena when the root's upload failed.)
    bool verify(bool root_ok, std::string& err) {
        if (comm.empty()) return root_ok;
        const size_t n = dev.size();
        std::vector<uint64_t> own(n, 0);
        bool hashed = true;
        for (size_t r = 0; r < n; ++r) {
            std::string e;
            if (!device_hash(dev[r], buf[r], bytes, &own[r], e)) { hashed = false; err = e; }
        }
        std::vector<unsigned long long*> w(n, nullptr);
        std::vector<DevPool> pools(n);  // one per rank: freed below with the rank's device current
        bool alloc = true;
        for (size_t r = 0; r < n; ++r) {
            (void)hipSetDevice(dev[r]);
            if (pools[r].alloc(w[r], 16) != hipSuccess) alloc = false;
        }
        // the root's words: status (0 ok), its arena hash; other ranks' buffers are overwritten
        const bool is_root = rank0;
        uint64_t msg[2] = {(root_ok && hashed) ? 0ull : 1ull, own[0]};
        for (size_t r = 0; r < n && alloc; ++r) {
            (void)hipSetDevice(dev[r]);
            if (hipMemcpy(w[r], msg, 16, hipMemcpyHostToDevice) != hipSuccess) alloc = false;
        }
        bool ok_all = alloc;
        if (alloc) {
            ncclResult_t nr = n > 1 ? ncclGroupStart() : ncclSuccess;
            for (size_t r = 0; r < n && nr == ncclSuccess; ++r) {
                (void)hipSetDevice(dev[r]);
                nr = ncclBroadcast(w[r], w[r], 16, ncclUint8, 0, comm[r], st[r]);
            }
            if (n > 1) {
                const ncclResult_t ne = ncclGroupEnd();
                if (nr == ncclSuccess) nr = ne;
            }
            if (nr != ncclSuccess) { ok_all = false; err = "status broadcast failed"; }
            for (size_t r = 0; r < n && ok_all; ++r) {
                (void)hipSetDevice(dev[r]);
                uint64_t got[2] = {1, 0};
                if (hipStreamSynchronize(st[r]) != hipSuccess ||
                    hipMemcpy(got, w[r], 16, hipMemcpyDeviceToHost) != hipSuccess) {
                    ok_all = false;
                    err = "status read back failed";
                } else if (got[0] != 0) {
                    ok_all = false;
                    if (err.empty()) err = is_root && r == 0 ? "the upload failed" : "the root rank's upload failed";
                } else if (!hashed || got[1] != own[r]) {
                    ok_all = false;
                    if (err.empty()) err = "arena hash of rank-local replica differs from the root's";
                }
            }
        } else if (err.empty()) {
            err = "status buffers";
        }
        for (size_t r = 0; r < n; ++r) {
            (void)hipSetDevice(dev[r]);
            pools[r].free_all();
        }
        (void)hipSetDevice(dev[0]);
        return ok_all;
    }
    bool rank0 = true;  // entry 0 is the communicator's root (in-process fan-outs, rank 0)
    // the model_load hook of the root: record the prefix on the upload stream, issue what it covers
    UploadHook hook() {
        return [this](size_t prefix_end, hipStream_t us) -> bool {
            hipEvent_t e = nullptr;
            (void)hipSetDevice(dev[0]);
            bool local = hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
            if (local) {
                evs.push_back(e);
                local = hipEventRecord(e, us) == hipSuccess;
            }
            if (!local) {  // no event to order the pieces behind the upload: wait for it here
                ok = false;
                (void)hipStreamSynchronize(us);
            }
            issue(prefix_end, local ? e : nullptr);
            (void)hipSetDevice(dev[0]);
            return ok;  // false aborts the upload; finish() still issues every remaining piece
        };
    }
};

bool check_replica_devices(int src, const int32_t* devices, int32_t n, const char* who) {
    const int nd = llmi_device_count();
    std::vector<int> seen{src};
    for (int i = 0; i < n; ++i) {
        if (devices[i] < 0 || devices[i] >= nd) { set_err(std::string(who) + ": device index out of range"); return false; }
        if (std::find(seen.begin(), seen.end(), devices[i]) != seen.end()) {
            set_err(std::string(who) + ": device " + std::to_string(devices[i]) +
                    " listed twice (or the source model's own device)");
            return false;
        }
        seen.push_back(devices[i]);
    }
    return true;
}

// in-process replicas: layouts on `devices`, one communicator over {src, devices...}
bool replica_setup(const Model& src, const int32_t* devices, int32_t n, std::vector<llama_model*>& reps, Fanout& F,
                   std::string& err) {
    reps.assign((size_t)n, nullptr);
    for (int i = 0; i < n; ++i) {
        reps[(size_t)i] = make_model([&](Model& M) { return model_clone_layout(src, devices[i], M, err); });
        if (!reps[(size_t)i]) return false;
    }
    F.dev.push_back(src.device);
    F.buf.push_back(src.arena);
    for (int i = 0; i < n; ++i) {
        F.dev.push_back(devices[i]);
        F.buf.push_back(reps[(size_t)i]->m.arena);
    }
    F.bytes = src.arena_bytes;
    F.comm.assign(F.dev.size(), nullptr);
    if (ncclCommInitAll(F.comm.data(), (int)F.dev.size(), F.dev.data()) != ncclSuccess) {
        F.comm.clear();
        err = "ncclCommInitAll failed";
        return false;
    }
    if (!F.make_streams()) { err = "replica streams"; return false; }
    return true;
}
}  // namespace

int32_t llmi_replicate(struct llama_model* model, const int32_t* devices, int32_t n, struct llama_model** out) {
    API_TRY
    if (!model || !devices || n <= 0 || !out) { set_err("llmi_replicate: bad arguments"); return -1; }
    // one RCCL rank per device: a device listed twice (or the source's own device) would
    // put two ranks of the communicator on one GPU
    if (!check_replica_devices(model->m.device, devices, n, "llmi_replicate")) return -1;
    std::vector<llama_model*> reps;
    std::string err;
    int rc = 0;
    {
        Fanout F;
        if (!replica_setup(model->m, devices, n, reps, F, err)) rc = -2;
        else if (!F.finish()) { err = "ncclBroadcast failed"; rc = -4; (void)F.verify(false, err); }
        else if (!F.verify(true, err)) rc = -6;
    }
    if (rc) {
        set_err("llmi_replicate: " + err);
        for (auto* r : reps) delete r;
        return rc;
    }
    for (int i = 0; i < n; ++i) out[i] = reps[(size_t)i];
    return 0;
    API_CATCH(-5)
}

struct llama_model* llmi_model_load_replicated(const char* path, struct llama_model_params params, const int32_t* devices,
                                               int32_t n, struct llama_model** out) {
    API_TRY
    if (!path || (n > 0 && (!devices || !out)) || n < 0 || params.vocab_only || params.no_upload) {
        set_err("llmi_model_load_replicated: bad arguments");
        return nullptr;
    }
    if (params.n_gpu_layers == 0) {
        set_err("llmi_model_load_replicated: n_gpu_layers=0 requests the CPU path; llmi is GPU-only");
        return nullptr;
    }
    const int nd = llmi_device_count();
    if (nd <= 0) { set_err("no HIP device visible"); return nullptr; }
    if (params.main_gpu < 0 || params.main_gpu >= nd) { set_err("main_gpu out of range"); return nullptr; }
    if (!check_replica_devices(params.main_gpu, devices, n, "llmi_model_load_replicated")) return nullptr;
    std::string err;
    // the layout first (no upload), then the replicas and the communicator, then the
    // upload with the pieces going out behind it
    llama_model* m = make_model([&](Model& M) {
        return model_load(path, params.main_gpu, false, true, M, err, nullptr, params.numerics);
    });
    if (!m) { set_err(err); return nullptr; }
    std::vector<llama_model*> reps;
    bool ok = true;
    {
        Fanout F;
        if (n > 0) ok = replica_setup(m->m, devices, n, reps, F, err);
        if (ok) {
            const UploadHook h = F.hook();
            ok = model_upload(m->m, err, n > 0 ? &h : nullptr);
            if (n > 0) {
                // every piece and the status go out even after a failed upload (every
                // replica learns it), then each replica's hash is checked against the root's
                const bool pieces = F.finish();
                if (ok && !pieces) { err = "ncclBroadcast failed"; ok = false; }
                std::string verr;
                if (!F.verify(ok, verr) && ok) { err = verr; ok = false; }
            }
        }
    }
    if (!ok) {
        set_err("llmi_model_load_replicated: " + err);
        for (auto* r : reps) delete r;
        delete m;
        return nullptr;
    }
    for (int i = 0; i < n; ++i) out[i] = reps[(size_t)i];
    return m;
    API_CATCH(nullptr)
}

int32_t llmi_rccl_unique_id(uint8_t* out, int32_t n) {
    if (!out || n < (int32_t)sizeof(ncclUniqueId)) { set_err("llmi_rccl_unique_id: buffer too small"); return -1; }
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) { set_err("ncclGetUniqueId failed"); return -2; }
    std::memcpy(out, &id, sizeof id);
    return 0;
}

namespace {
bool proc_fanout_init(Fanout& F, const Model& m, const uint8_t* uid, int32_t nranks, int32_t rank) {
    (void)hipSetDevice(m.device);
    ncclUniqueId id;
    std::memcpy(&id, uid, sizeof id);
    F.dev = {m.device};
    F.buf = {m.arena};
    F.bytes = m.arena_bytes;
    F.comm.assign(1, nullptr);
    if (ncclCommInitRank(&F.comm[0], nranks, id, rank) != ncclSuccess) {
        F.comm.clear();
        set_err("ncclCommInitRank failed");
        return false;
    }
    if (!F.make_streams()) { set_err("fan-out stream"); return false; }
    return true;
}
}  // namespace

int32_t llmi_model_fanout(struct llama_model* model, const uint8_t* uid, int32_t nranks, int32_t rank) {
    API_TRY
    if (!model || !uid || nranks <= 0 || rank < 0 || rank >= nranks || !model->m.arena) {
        set_err("llmi_model_fanout: bad arguments");
        return -1;
    }
    if (nranks == 1) return 0;
    Fanout F;
    if (!proc_fanout_init(F, model->m, uid, nranks, rank)) return -2;
    F.rank0 = rank == 0;
    const bool pieces = F.finish();
    std::string err;
    if (!F.verify(pieces || rank != 0, err)) { set_err("llmi_model_fanout: " + err); return pieces ? -6 : -3; }
    if (!pieces) { set_err("llmi_model_fanout: broadcast failed"); return -3; }
    return 0;
    API_CATCH(-5)
}

struct llama_model* llmi_model_load_fanout(const char* path, struct llama_model_params params, const uint8_t* uid,
                                           int32_t nranks, int32_t rank) {
    API_TRY
    if (!path || !uid || nranks <= 0 || rank < 0 || rank >= nranks || params.vocab_only) {
        set_err("llmi_model_load_fanout: bad arguments");
        return nullptr;
    }
    if (params.n_gpu_layers == 0) {
        set_err("llmi_model_load_fanout: n_gpu_layers=0 requests the CPU path; llmi is GPU-only");
        return nullptr;
    }
    const int nd = llmi_device_count();
    if (nd <= 0) { set_err("no HIP device visible"); return nullptr; }
    if (params.main_gpu < 0 || params.main_gpu >= nd) { set_err("main_gpu out of range"); return nullptr; }
    std::string err;
    llama_model* m = make_model([&](Model& M) {
        return model_load(path, params.main_gpu, false, true, M, err, nullptr, params.numerics);
    });
    if (!m) { set_err(err); return nullptr; }
    bool ok = true;
    if (nranks > 1) {
        Fanout F;
        ok = proc_fanout_init(F, m->m, uid, nranks, rank);
        F.rank0 = rank == 0;
        if (ok && rank == 0) {
            const UploadHook h = F.hook();
            ok = model_upload(m->m, err, &h);
            if (!ok) set_err(err);
        }
        // every piece is issued even after a failed upload: the other ranks are blocked in
        // their matching broadcasts and would otherwise never return
        if (!F.comm.empty()) {
            const bool pieces = F.finish();
            if (!pieces && ok) { set_err("llmi_model_load_fanout: broadcast failed"); ok = false; }
            // then the root's status + arena hash: a rank whose root failed (or whose
            // replica differs) returns NULL instead of a partly written arena
            std::string verr;
            if (!F.verify(rank == 0 ? ok : true, verr) && ok) {
                set_err("llmi_model_load_fanout: " + verr);
                ok = false;
            }
        }
    } else {
        ok = model_upload(m->m, err, nullptr);
        if (!ok) set_err(err);
    }
    if (!ok) {
        delete m;
        return nullptr;
    }
    return m;
    API_CATCH(nullptr)
}

int32_t llmi_fanout_plan(uint64_t arena_bytes, uint64_t chunk, const uint64_t* prefix_ends, int32_t n_prefix,
                         int32_t* ready, int32_t max_pieces) {
    if (n_prefix < 0 || (n_prefix > 0 && !prefix_ends) || max_pieces < 0 || (max_pieces > 0 && !ready)) return -1;
    API_TRY
    std::vector<size_t> pe(prefix_ends, prefix_ends + n_prefix);
    std::vector<int> rd;
    const size_t n = fanout_plan((size_t)arena_bytes, (size_t)chunk, pe, rd);
    for (size_t k = 0; k < n && (int32_t)k < max_pieces; ++k) ready[k] = rd[k];
    return (int32_t)n;
    API_CATCH(-5)
}

}  // extern "C"
