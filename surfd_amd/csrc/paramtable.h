// The parameter table of the network handles (decoder.hip, unet.hip, dgcnn.hip, xattn.hip), included after common.h.  Host code
// only, no HIP calls: which tensors a checkpoint must bring, in state_dict order, their shapes, and which of them have arrived.
// Where a tensor goes on the device (pack_matrix, pack_segment, the CBN index, pblock + tag) is each handle's own.
//
// Every surfd_*_set_param checks in ONE order: null handle; match() (key, rank, dimensions); an ignored entry
// (num_batches_tracked) is marked and returns SURFD_OK, a null pointer is fine for it; a null dev_ptr is SURFD_ERR_ARG; the
// handle's lazy allocation; copy or pack; mark() and finalized = false.  Against the four copies this table replaced:
//   1. the encoder checks the shape before it allocates (a wrong dimension used to cost a hipMalloc, and answered
//      SURFD_ERR_HIP on a host without a GPU);
//   2. the decoder's finalize no longer requires num_batches_tracked, which was the encoder's rule already: it accepts more,
//      never less;
//   3. a call that is wrong in two ways may name the other fault first.
// The return code of every singly-wrong call is what it was.
#pragma once
#include <initializer_list>

namespace surfd {

struct ParamEntry {
    std::string key;
    int64_t shape[4] = {0, 0, 0, 0};
    int ndim = 0;
    bool ignored = false;        // num_batches_tracked: matched like any other entry (rank 0), never copied, never missing
    bool is_set = false;
    long tag = 0;                // the owner's: the encoder's float offset into pblock, cross-attention's pointer index
};

struct ParamTable {
    std::vector<ParamEntry> entries;
    std::map<std::string, int> index;

    int add(const std::string &key, std::initializer_list<int64_t> shape, long tag = 0, bool ignored = false) {
        ParamEntry e;
        e.key = key;
        for (int64_t v : shape) e.shape[e.ndim++] = v;
        e.ignored = ignored;
        e.tag = tag;
        index[key] = (int)entries.size();
        entries.push_back(e);
        return (int)entries.size() - 1;
    }
    int size() const { return (int)entries.size(); }
    const ParamEntry &operator[](int i) const { return entries[i]; }
    size_t numel(int i) const {
        size_t n = 1;
        for (int j = 0; j < entries[i].ndim; ++j) n *= (size_t)entries[i].shape[j];
        return n;
    }

    // key -> *which, after the rank and every dimension agree
    int match(const char *who, const char *key, const int64_t *shape, int ndim, int *which) const {
        if (!key) SURFD_FAIL(SURFD_ERR_ARG, "%s: null key", who);
        auto it = index.find(key);
        if (it == index.end()) SURFD_FAIL(SURFD_ERR_ARG, "%s: unknown key '%s'", who, key);
        const ParamEntry &e = entries[it->second];
        if (ndim != e.ndim) SURFD_FAIL(SURFD_ERR_ARG, "%s: '%s' has rank %d, expected %d", who, key, ndim, e.ndim);
        if (ndim > 0 && !shape) SURFD_FAIL(SURFD_ERR_ARG, "%s: '%s' has a null shape", who, key);
        for (int j = 0; j < ndim; ++j)
            if (shape[j] != e.shape[j])
                SURFD_FAIL(SURFD_ERR_ARG, "%s: '%s' dim %d is %lld, expected %lld", who, key, j, (long long)shape[j], (long long)e.shape[j]);
        *which = it->second;
        return SURFD_OK;
    }
    void mark(int i) { entries[i].is_set = true; }
    int first_missing() const {
        for (int i = 0; i < size(); ++i)
            if (!entries[i].is_set && !entries[i].ignored) return i;
        return -1;
    }
    bool all_set() const { return first_missing() < 0; }
    // what finalize (cross-attention: forward) asks before it reads the device copies
    int require_all(const char *who) const {
        const int m = first_missing();
        if (m >= 0) SURFD_FAIL(SURFD_ERR_STATE, "%s: parameter '%s' was not set", who, entries[m].key.c_str());
        return SURFD_OK;
    }
};

// the body of surfd_*_param_info; t is null where the handle was
static inline int param_info(const ParamTable *t, const char *who, int i, const char **key, int64_t shape[4], int *ndim) {
    if (!t || i < 0 || i >= t->size() || !key || !shape || !ndim) SURFD_FAIL(SURFD_ERR_ARG, "%s: null argument or bad index %d", who, i);
    const ParamEntry &e = (*t)[i];
    *key = e.key.c_str();
    *ndim = e.ndim;
    for (int j = 0; j < e.ndim; ++j) shape[j] = e.shape[j];
    return SURFD_OK;
}

}  // namespace surfd
