// An owning, grow-only buffer for the handle's device and pinned allocations (cnf_abi_int.h), and the one table of Runge-Kutta
// coefficients the adjoint's host code reads.
//
// Plain C++ (no HIP): the allocator is a policy with static `int alloc(void**, size_t bytes)` (0 = success) and
// `void free(void*)`; cnf_abi_int.h instantiates it over hipMalloc / hipFree and hipHostMalloc / hipHostFree,
// tests/support/buf_test.cpp over a counting fake.
#pragma once
#include <cstddef>

template <class T, class Alloc>
class CnfBuf {
    T* p_ = nullptr;
    size_t cap_ = 0;          // elements

public:
    CnfBuf() = default;
    CnfBuf(const CnfBuf&) = delete;
    CnfBuf& operator=(const CnfBuf&) = delete;
    ~CnfBuf() { release(); }

    // Room for n elements; the contents are NOT kept.  Within capacity: nothing is called.  Otherwise the old allocation is
    // released first, then n * sizeof(T) bytes are asked for: the buffer ends holding n elements, or empty with the
    // allocator's error returned -- never with a pointer that has been freed.
    int reserve(size_t n) {
        if (n <= cap_) return 0;
        release();
        void* q = nullptr;
        const int e = Alloc::alloc(&q, n * sizeof(T));
        if (e != 0) return e;
        p_ = static_cast<T*>(q);
        cap_ = n;
        return 0;
    }
    void release() {
        if (p_) Alloc::free(p_);
        p_ = nullptr;
        cap_ = 0;
    }
    // (growth that keeps the contents is the caller's: reserve a second buffer, copy, swap -- traj_reserve)
    void swap(CnfBuf& o) {
        T* p = p_; p_ = o.p_; o.p_ = p;
        const size_t c = cap_; cap_ = o.cap_; o.cap_ = c;
    }
    T* data() const { return p_; }
    operator T*() const { return p_; }       // reads like the raw pointer it replaces; it cannot be assigned like one
    size_t capacity() const { return cap_; }
};

// The Tsit5 tableau as the discrete adjoint reads it.  `row(s, r)` is tsit5_row (cnf_dev.h): r[0..5] = a_{s+1, 1..6}, row 6 = b.
struct AdjTableau {
    float a[6][5];      // a[m][i]: weight of k_{i+1} in the state of stage m + 1 (the per-stage pullback)
    float b[6];
    float kc[6][5];     // kc[m][d] = a[m][m - 1 - d]: the same rows as the one-launch pullback kernels walk them, 0 beyond
};
template <class RowFn>
inline AdjTableau adj_tableau(RowFn row) {
    AdjTableau t{};
    float r[6];
    for (int m = 0; m < 6; ++m) {
        row(m, r);
        for (int i = 0; i < 5; ++i) t.a[m][i] = r[i];
    }
    row(6, r);
    for (int i = 0; i < 6; ++i) t.b[i] = r[i];
    for (int m = 0; m < 6; ++m)
        for (int d = 0; d < 5; ++d) t.kc[m][d] = m - 1 - d >= 0 ? t.a[m][m - 1 - d] : 0.f;
    return t;
}
