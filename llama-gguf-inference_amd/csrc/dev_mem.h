// dev_mem.h — DevPool, the owner of device and pinned host memory: whatever is allocated
// through a pool is freed by it, so the allocation is the registration.  A Context owns one
// for its whole life (engine.h); a hook or fan-out call owns a local one for its duration.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <initializer_list>
#include <vector>

namespace llmi {

struct DevPool {
    std::vector<void*> dev, pinned;
    hipError_t err = hipSuccess;  // get(): the first error, which fails every later get()

    // A block of `bytes`, not zeroed (the owner orders any memset with its own stream); p is
    // null after a failure, which leaves the pool as it was: an optional block may fail.
    template <class T>
    hipError_t alloc(T*& p, size_t bytes) {
        void* v = nullptr;
        const hipError_t e = hipMalloc(&v, bytes);
        if (e == hipSuccess) dev.push_back(v);
        p = (T*)v;
        return e;
    }
    template <class T>
    hipError_t alloc_pinned(T*& p, size_t bytes) {
        void* v = nullptr;
        const hipError_t e = hipHostMalloc(&v, bytes, hipHostMallocDefault);
        if (e == hipSuccess) pinned.push_back(v);
        p = (T*)v;
        return e;
    }
    // One hook call's allocations (null stream): zeroed unless told otherwise; after a failure
    // every further request returns null and `err` keeps the first error.
    template <class T>
    T* get(size_t bytes, bool zero = true) {
        T* p = nullptr;
        if (err == hipSuccess) err = alloc(p, bytes ? bytes : 1);
        if (err != hipSuccess) return nullptr;
        if (zero) err = hipMemset(p, 0, bytes);
        return p;
    }
    void release(void* p) {
        auto it = std::find(dev.begin(), dev.end(), p);
        if (it != dev.end()) { (void)hipFree(p); dev.erase(it); return; }
        it = std::find(pinned.begin(), pinned.end(), p);
        if (it != pinned.end()) { (void)hipHostFree(p); pinned.erase(it); }
    }
    // Grow on demand.  The blocks share the capacity `cap` (block b holds cap * b.elem bytes):
    // nothing happens while cap covers `need`; else the old blocks are released (after a
    // synchronize of `sync`, when given: work in flight may still use them) and blocks of
    // `count` elements allocated.  After a failure every pointer is null and cap is 0.
    struct Block {
        void** p;
        size_t elem;
        bool pin;
        template <class T>
        Block(T** p_, size_t elem_, bool pin_ = false) : p((void**)p_), elem(elem_), pin(pin_) {}
    };
    template <class Cap>
    hipError_t grow(std::initializer_list<Block> blocks, Cap& cap, size_t need, size_t count, hipStream_t sync = nullptr) {
        if (need <= (size_t)cap) return hipSuccess;
        hipError_t e = sync ? hipStreamSynchronize(sync) : hipSuccess;
        if (e != hipSuccess) return e;
        cap = 0;
        for (const Block& b : blocks) {
            release(*b.p);
            *b.p = nullptr;
        }
        for (const Block& b : blocks) {
            if (e == hipSuccess) e = b.pin ? alloc_pinned(*b.p, count * b.elem) : alloc(*b.p, count * b.elem);
        }
        if (e == hipSuccess) cap = (Cap)count;
        else
            for (const Block& b : blocks) {
                release(*b.p);
                *b.p = nullptr;
            }
        return e;
    }
    // with the memory's device current (a Context's destructor calls it inside its device scope)
    void free_all() {
        for (void* p : dev) (void)hipFree(p);
        for (void* p : pinned) (void)hipHostFree(p);
        dev.clear();
        pinned.clear();
    }
    DevPool() = default;
    DevPool(const DevPool&) = delete;
    DevPool& operator=(const DevPool&) = delete;
    ~DevPool() { free_all(); }
};

}  // namespace llmi
