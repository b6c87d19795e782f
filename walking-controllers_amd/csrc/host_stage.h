// Where a *_host entry point's arrays sit in its one block of device memory.  The entry point names each array ONCE - host pointer,
// element count, direction - and the offset, the block's size, the copy in and the copy out all follow from that statement
// (wcqp::HostStage in wcqp_internal.h puts the copies on top).  Plain host arithmetic: no HIP header, no heap.
#pragma once
#include <cstddef>

namespace wcqp {

template <class T>
struct StageSlot { int row = -1; };        // -1: the device sees NULL

constexpr int kStageRefused = -1;           // (WCQP_E_INVALID)

struct StageLayout {
    static constexpr int kMaxRows = 16;   // the IK form stages 12 arrays, prepare 11, the unicycle planner 10 (timed: 12)
    struct Row { const void* src; void* dst; size_t off, bytes; };     // src: copied in; dst: copied out (NULL: the caller does not want it back)
    Row rows[kMaxRows];
    int n = 0;
    size_t total = 0;                      // bytes of the block
    bool refused = false;                  // a 17th array, or an input without its host array: nothing is reserved or copied
    char* base = nullptr;                  // the block, once there is one

    // An array is packed behind the one before it, aligned to its own element size and to nothing more: with an odd batch the kernels
    // see arrays that are only 8-byte aligned, as they do from callers of the *_device forms.  `null_when_absent`: without a host
    // array (or with no elements) the array takes no room and the device form is handed NULL; an output without the flag keeps its
    // device array when the caller does not want it back.
    template <class T> StageSlot<T> in(const T* host, size_t count, bool null_when_absent = false) {
        return {add(host, nullptr, true, count, sizeof(T), null_when_absent)};
    }
    template <class T> StageSlot<T> out(T* host, size_t count, bool null_when_absent = false) {
        return {add(nullptr, host, false, count, sizeof(T), null_when_absent)};
    }
    template <class T> StageSlot<T> inout(T* host, size_t count, bool null_when_absent = false) {
        return {add(host, host, true, count, sizeof(T), null_when_absent)};
    }
    template <class T> size_t offset(StageSlot<T> s) const { return rows[s.row].off; }
    template <class T> T* operator[](StageSlot<T> s) const { return s.row < 0 ? nullptr : reinterpret_cast<T*>(base + rows[s.row].off); }
    // a block of `capacity` bytes holds this layout
    bool fits(size_t capacity) const { return !refused && total <= capacity; }
    // The copies, whatever copies: copy(dst, src, bytes) returns 0 or the error the call ends with.  copy_in takes the block and fills
    // every input's rows - a layout that was refused or does not fit leaves the block unwritten (kStageRefused); copy_out hands back
    // every output the caller gave a host array for.
    template <class Copy> int copy_in(void* block, size_t capacity, Copy&& copy) {
        if (!block || !fits(capacity)) return kStageRefused;
        base = static_cast<char*>(block);
        for (int k = 0; k < n; ++k)
            if (rows[k].src && rows[k].bytes)
                if (const int e = copy(base + rows[k].off, rows[k].src, rows[k].bytes)) return e;
        return 0;
    }
    template <class Copy> int copy_out(Copy&& copy) const {
        for (int k = 0; k < n; ++k)
            if (rows[k].dst && rows[k].bytes)
                if (const int e = copy(rows[k].dst, base + rows[k].off, rows[k].bytes)) return e;
        return 0;
    }

private:
    int add(const void* src, void* dst, bool is_input, size_t count, size_t elem, bool null_when_absent) {
        const bool given = is_input ? src != nullptr : dst != nullptr;
        if (null_when_absent && (!given || count == 0)) return -1;
        if (n == kMaxRows || (is_input && !given)) { refused = true; return -1; }
        const size_t off = (total + elem - 1) / elem * elem;
        rows[n] = Row{src, dst, off, count * elem};
        total = off + count * elem;
        return n++;
    }
};

// a host pointer that stands for "present" where a layout is only sized (every optional array there, nothing copied)
alignas(8) inline constexpr unsigned char kStageSizing[8] = {};
template <class T> const T* stage_sizing() { return reinterpret_cast<const T*>(kStageSizing); }

}  // namespace wcqp
