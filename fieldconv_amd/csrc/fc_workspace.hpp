// Caller-owned buffers (workspaces, `saved`): every piece starts on a 256-byte boundary, and each buffer has ONE layout function
// that takes its pieces from a Carver.  Run on a null Carver the function only measures, and `used` is what the *_bytes query
// returns; run on the caller's pointer it hands out the pieces.  The size and the carve are therefore the same statement.
#pragma once
#include <cstddef>
#include <cstdint>

namespace fc {

inline size_t align256(size_t v) { return (v + 255) / 256 * 256; }

struct Carver {
    char* base;
    size_t used = 0;            // offset of the next piece; after the last take, the size of the buffer
    explicit Carver(const void* p = nullptr) : base(static_cast<char*>(const_cast<void*>(p))) {}
    // room: where wanted, the bytes the piece occupies (for a piece that is handed on as another entry point's workspace)
    template <typename T = void>
    T* take(size_t bytes, size_t* room = nullptr) {
        if (room) *room = align256(bytes);
        return take_packed<T>(align256(bytes));
    }
    // no rounding: the convolution's backward workspaces are older than the 256-byte rule, and their pieces stay back to back
    template <typename T = void>
    T* take_packed(size_t bytes) {
        T* r = base ? reinterpret_cast<T*>(base + used) : nullptr;
        used += bytes;
        return r;
    }
};

// the size of a buffer: its layout function run on a null Carver
template <typename F, typename... A>
size_t carved_bytes(F layout, const A&... a) {
    Carver c;
    layout(c, a...);
    return c.used;
}

// The head of FCPrecomp's workspace: the selection fc_precomp_mark leaves behind, read by fc_precomp_build (csrc/fc_precomp.hip) and by
// the fused fc_precomp_graph (csrc/fc_graph.hip).  keep and pos hold E+2 int32 each: pos[E] = number of kept edges, pos[E+1] = the
// index-range flag; total: the per-vertex area sums (N floats, last, so keep and pos lie where E alone puts them).
struct PrecompSelection { int32_t *keep, *pos; float* total; };
inline PrecompSelection precomp_selection(Carver& c, int N, int E) {
    return {c.take<int32_t>((size_t)(E + 2) * 4), c.take<int32_t>((size_t)(E + 2) * 4), c.take<float>((size_t)N * 4)};
}

}  // namespace fc
