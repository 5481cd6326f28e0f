// Host scaffolding shared by the five generator engines (unet.hip, pan.hip, ppon.hip, resnet.hip, wbcunet.hip): the parameter table behind
// innfer_<eng>_num_params / _param_info / _set_param, and the owner of an engine's device allocations.  Host code only.
#pragma once
#include "common.h"

#include <cstring>

namespace innfer {

struct Param { std::string key; std::vector<int> shape; std::vector<float> host; bool set = false; };

// The state-dict entries of a network in module order.  `eng` is the engine's name as its error texts spell it ("unet", "pan", ...).
struct ParamTable {
    std::vector<Param> v;

    int add(const std::string& key, std::vector<int> shape) {
        Param p; p.key = key; p.shape = std::move(shape);
        v.push_back(std::move(p));
        return (int)v.size() - 1;
    }
    int find(const std::string& key) const {
        for (size_t i = 0; i < v.size(); ++i) if (v[i].key == key) return (int)i;
        return -1;
    }
    Param& operator[](size_t i) { return v[i]; }
    const Param& operator[](size_t i) const { return v[i]; }
    size_t size() const { return v.size(); }
    std::vector<Param>::const_iterator begin() const { return v.begin(); }
    std::vector<Param>::const_iterator end() const { return v.end(); }

    // the table of a handle; a null handle has the empty table, in which every index is a bad one
    template <class E> static ParamTable& of(E* e) { static ParamTable none; return e ? e->params : none; }

    int info(const char* eng, int idx, char* key, size_t cap, int* ndim, int* shape4) const {
        if (idx < 0 || idx >= (int)v.size()) return set_error(INNFER_ERR_INVALID, "%s_param_info: bad index", eng);
        const Param& p = v[idx];
        if (key && cap) { strncpy(key, p.key.c_str(), cap - 1); key[cap - 1] = 0; }
        if (ndim) *ndim = (int)p.shape.size();
        if (shape4) for (size_t i = 0; i < 4; ++i) shape4[i] = i < p.shape.size() ? p.shape[i] : 1;
        return INNFER_OK;
    }
    int set(const char* eng, int idx, const float* data) {
        if (idx < 0 || idx >= (int)v.size() || !data) return set_error(INNFER_ERR_INVALID, "%s_set_param: bad arguments", eng);
        Param& p = v[idx];
        size_t n = 1;
        for (int s : p.shape) n *= (size_t)s;
        p.host.assign(data, data + n);
        p.set = true;
        return INNFER_OK;
    }
    // statistics_optional: a checkpoint may lack BatchNorm's buffers (running_mean / running_var / num_batches_tracked)
    int require_all_set(const char* eng, bool statistics_optional) const {
        for (const Param& p : v) {
            if (p.set) continue;
            if (statistics_optional && (p.key.find("running_") != std::string::npos || p.key.find("num_batches") != std::string::npos)) continue;
            return set_error(INNFER_ERR_INVALID, "%s: parameter '%s' was never set", eng, p.key.c_str());
        }
        return INNFER_OK;
    }
};

// The one owner of an engine's device allocations: put() allocates, copies and records; clear() (and the destructor) frees.  The pointers an engine
// keeps in its records are views of these blocks -- it value-resets the records after clear() and never frees one itself.
struct DeviceBufs {
    std::vector<void*> blocks;

    DeviceBufs() = default;
    DeviceBufs(const DeviceBufs&) = delete;
    DeviceBufs& operator=(const DeviceBufs&) = delete;
    ~DeviceBufs() { clear(); }

    template <class T>
    int put(T** dst, const void* host, size_t bytes) {          // *dst is written only when the block holds the data
        void* d = nullptr;
        INNFER_HIP(hipMalloc(&d, bytes));
        const hipError_t copied = hipMemcpy(d, host, bytes, hipMemcpyHostToDevice);
        if (copied != hipSuccess) (void)hipFree(d);
        INNFER_HIP(copied);
        blocks.push_back(d);
        *dst = (T*)d;
        return INNFER_OK;
    }
    template <class T, class V>
    int put(T** dst, const std::vector<V>& host) { return put(dst, host.data(), host.size() * sizeof(V)); }

    void clear() {
        for (void* b : blocks) (void)hipFree(b);
        blocks.clear();
    }
};

}  // namespace innfer
