// sampler_side.h -- what a logit stage keeps beside a Sampler (the Sampler struct is the reference's: settings live beside it, keyed by its address) and
// the small device block its launch reads. A block is rewritten in stream order when the host changes a value, so a captured graph never holds a value
// of it -- only its address. q4_logit_process.hip, q4_dry.hip and q4_adaptive.hip each keep one SamplerSides of their own record type; their
// op-level launchers keep one DeviceBlock.
#pragma once
#include <map>
#include "q4_model.h"

namespace q4 {

template <class P>
struct DeviceBlock {
    P host;                            // what the next upload sends (pageable: the copy call returns when it has been staged)
    P* dev = nullptr;
    bool dirty = true;                 // the device block is behind the host's values: the owner fills `host` before upload()
    bool stale() const { return dirty || !dev; }
    // allocated once; copied, in stream order, when stale
    int upload() {
        if (!dev) {
            Q4_HIP(hipMalloc((void**)&dev, sizeof(P)));
            dirty = true;
        }
        if (dirty) {
            Q4_HIP(hipMemcpyAsync(dev, &host, sizeof(P), hipMemcpyHostToDevice, g_stream));
            dirty = false;
        }
        return Q4_OK;
    }
    void release() {
        if (dev) (void)hipFree(dev);
        dev = nullptr;
    }
};

// R: a DeviceBlock with the settings it is filled from and `bool on() const`
template <class R>
struct SamplerSides {
    std::map<const Sampler*, R> records;
    R* find(const Sampler* sampler) {                          // never creates a record
        auto it = records.find(sampler);
        return it == records.end() ? nullptr : &it->second;
    }
    R& of(const Sampler* sampler) { return records[sampler]; }
    bool on(const Sampler* sampler) {
        if (!sampler || records.empty()) return false;
        const R* r = find(sampler);
        return r && r->on();
    }
    const void* block(const Sampler* sampler) {
        const R* r = find(sampler);
        return r ? r->dev : nullptr;
    }
    // destroy_sampler: the caller has dropped the graphs that hold the block and drained the stream
    void forget(const Sampler* sampler) {
        auto it = records.find(sampler);
        if (it == records.end()) return;
        it->second.release();
        records.erase(it);
    }
};

}  // namespace q4
