// The workspace of a host-composed step (fusion_model.hip with legacy_vqa.inc, pretrain_model.hip): one caller-owned
// block carved into named buffers.  The layout is a function of the dims alone, so the host views named intermediates
// without copies (the *_tensor entry points) and a backward finds what its forward left.  Internal: not part of the C ABI.
#pragma once
#include <stdint.h>

#include <string>
#include <string_view>
#include <vector>

struct Entry { std::string name; int64_t off, n; };      // byte offset, element count

struct Layout {
    std::vector<Entry> e;
    int64_t total = 0;
    void add(const std::string& name, int64_t n, int esz = 4) {
        e.push_back({name, total, n});
        total += ((n * esz + 255) / 256) * 256;      // 256-byte aligned carve
    }
    // a named view of `cnt` floats inside an existing entry of FLOATS (the stacked heads' tensors are slices of one block)
    void alias(const std::string& name, std::string_view base, int64_t off_floats, int64_t cnt) {
        e.push_back({name, find(base)->off + off_floats * 4, cnt});
    }
    // NULL for a name the layout does not have: the *_tensor entry points' answer to an unknown name, and how a step asks
    // for a buffer that exists only for some shapes ("gru_ws")
    const Entry* find(std::string_view name) const {
        for (const auto& x : e)
            if (x.name == name) return &x;
        return nullptr;
    }
};

// A layout over a caller's block.  Precondition of f / i32 / u16 / count: the layout has the name (a step names only
// buffers its own layout function added for the dims at hand); find_f is for the names that depend on the shape.
struct Workspace {
    const Layout& L;
    char* ws;
    float* f(std::string_view name) const { return reinterpret_cast<float*>(ws + L.find(name)->off); }
    int32_t* i32(std::string_view name) const { return reinterpret_cast<int32_t*>(ws + L.find(name)->off); }
    uint16_t* u16(std::string_view name) const { return reinterpret_cast<uint16_t*>(ws + L.find(name)->off); }
    int64_t count(std::string_view name) const { return L.find(name)->n; }
    float* find_f(std::string_view name) const { return L.find(name) ? f(name) : nullptr; }
};
