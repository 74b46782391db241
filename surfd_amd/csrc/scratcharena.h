// The temporaries of one call (or of one stage of a call), carved from ONE block: a block per temporary is a hipMalloc / hipFree
// pair each, and a call of meshclean.hip has up to fourteen.  Plain C++ after common.h, no HIP call: the
// stand-alone check tools/scratcharena_check.cpp adopts a host block and carves the slot sequences of the call sites from it.
//   dev_slot<T>(n)      the bytes of a slot of max(n, 1) elements: a multiple of 256, so every slot starts 256-byte aligned.
//   open(scratch, b)    takes one block of b bytes from the call's DeviceScratch: the sum of the slots the stage is going to ask for.
//                       An arena may be opened again for a later stage; the earlier block lives on with the scratch.
//   adopt(base, b)      the same over a block the caller owns.
//   get(&ptr, n)        the next slot; SURFD_ERR_STATE past the end, under the name the arena was made with.
#pragma once
#include <cstddef>

namespace surfd {

template <class T>
static inline size_t dev_slot(long n) { return ((size_t)(n > 1 ? n : 1) * sizeof(T) + 255) & ~(size_t)255; }

class ScratchArena {
    const char *who;
    char *base = nullptr;
    size_t size = 0, used = 0;
  public:
    explicit ScratchArena(const char *who) : who(who) {}
    void adopt(void *block, size_t bytes) {
        base = (char *)block;
        size = bytes; used = 0;
    }
    template <class Scratch>
    int open(Scratch &scratch, size_t bytes) {
        adopt(nullptr, bytes);
        return scratch.get(&base, (long)bytes);
    }
    template <class T>
    int get(T **ptr, long n) {
        const size_t b = dev_slot<T>(n);
        if (used + b > size) SURFD_FAIL(SURFD_ERR_STATE, "%s: the arena of the call is too small (%zu + %zu > %zu bytes)", who, used, b, size);
        *ptr = (T *)(base + used);
        used += b;
        return SURFD_OK;
    }
};

}  // namespace surfd
