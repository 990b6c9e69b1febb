// Host-side layout of one device allocation (model.hip, vae.hip: model weights and activation workspaces).  Regions are taken in order,
// each 256-byte aligned; a region names the pointer field it will be bound to, and bind() sets every such field once the allocation
// exists.  A region that is not taken leaves its field null.  Not included by any kernel translation unit.
#pragma once
#include <cstddef>
#include <cstring>
#include <vector>

namespace dd {

// fp32 -> bf16 bits, round-to-nearest-even (the host image of a bf16 weight; f2bf's rounding)
inline unsigned short host_f2bf(float f) {
    unsigned u;
    std::memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40);  // NaN stays NaN
    return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

class Arena {
public:
    explicit Arena(size_t esize = 4) : es_(esize) {}

    // fp32 vector
    template <typename P> void f32(P*& field, const float* src, size_t n) { std::memcpy(data(field, n * 4), src, n * 4); }
    template <typename P> void f32(P*& field, const std::vector<float>& v) { f32(field, v.data(), v.size()); }
    // matrix in the element size of the arena: fp32, or bf16 through host_f2bf
    template <typename P> void mat(P*& field, const std::vector<float>& v) {
        char* d = data(field, v.size() * es_);
        if (es_ == 4) std::memcpy(d, v.data(), v.size() * 4);
        else for (size_t i = 0; i < v.size(); ++i) ((unsigned short*)d)[i] = host_f2bf(v[i]);
    }
    // zero-filled region for a packer to fill: the host pointer is valid until the next region is taken
    template <typename P> char* raw(P*& field, size_t bytes) { return data(field, bytes); }
    // size only (workspaces: no host image)
    template <typename P> void space(P*& field, size_t bytes) { take(field, bytes); }

    size_t bytes() const { return off_; }
    const char* image() const { return img_.data(); }   // the host image of the data regions (bytes() long when only data regions were taken)
    void bind(char* base) const {
        for (const Slot& s : slots_) s.set(s.field, base + s.off);
    }

private:
    struct Slot { void* field; size_t off; void (*set)(void*, char*); };
    template <typename P> static void set(void* field, char* p) { *static_cast<P**>(field) = static_cast<P*>(static_cast<void*>(p)); }

    template <typename P> size_t take(P*& field, size_t bytes) {
        const size_t o = off_;
        off_ += (bytes + 255) / 256 * 256;
        slots_.push_back(Slot{&field, o, &set<P>});
        return o;
    }
    template <typename P> char* data(P*& field, size_t bytes) {
        const size_t o = take(field, bytes);
        img_.resize(off_, 0);
        return img_.data() + o;
    }

    size_t es_;
    size_t off_ = 0;
    std::vector<char> img_;
    std::vector<Slot> slots_;
};

}  // namespace dd
