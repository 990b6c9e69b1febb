// Kernel tables: one entry per instantiation of a templated kernel that needs the dynamic-LDS opt-in.  A family's table is the only
// place that names its instantiations: the dispatcher finds its kernel there, the opt-in walks it, the *_supported predicates ask it
// which widths exist.  A new instantiation is one line in its table.
#pragma once
#include <hip/hip_runtime.h>

#include <array>
#include <iterator>
#include <vector>

namespace dd {

struct KernelInfo {
    std::array<int, 4> key;     // the template arguments the dispatcher selects by (unused slots 0)
    const void* fn;
    int block;
    int lds_max;                // dynamic-LDS ceiling the kernel is opted in to; no launch may ask for more
};

// ... + the typed launcher: its parameters are the kernel's own, so an entry made from a kernel of another signature does not compile
template <typename... P>
struct KernelEntry : KernelInfo {
    void (*run)(dim3 grid, dim3 block, size_t lds, hipStream_t s, P... args);
};

template <auto Kernel, typename... P>
void run_kernel(dim3 grid, dim3 block, size_t lds, hipStream_t s, P... args) {
    hipLaunchKernelGGL(Kernel, grid, block, lds, s, args...);
}
template <auto Kernel, typename... P>
KernelEntry<P...> entry_of(void (*)(P...), std::array<int, 4> key, int block, size_t lds_max) {
    return {{key, (const void*)Kernel, block, (int)lds_max}, run_kernel<Kernel, P...>};
}
template <auto Kernel>
auto entry(std::array<int, 4> key, int block, size_t lds_max) { return entry_of<Kernel>(Kernel, key, block, lds_max); }

template <typename Table>
auto find(const Table& table, int k0, int k1 = 0, int k2 = 0, int k3 = 0) -> decltype(std::begin(table)) {
    for (const auto& e : table)
        if (e.key == std::array<int, 4>{k0, k1, k2, k3}) return &e;
    return nullptr;
}

// no entry (find's null), or more LDS than the entry is opted in to: refused before anything reaches the device
template <typename... P, typename... A>
hipError_t launch(const KernelEntry<P...>* e, dim3 grid, size_t lds, hipStream_t s, const A&... args) {
    if (!e || lds > (size_t)e->lds_max) return hipErrorInvalidValue;
    e->run(grid, dim3(e->block), lds, s, args...);
    return hipGetLastError();
}

// a table without its argument types, for the opt-in and the listing: the kernel's name, entry i or null past the end.  family<kTable>("name"),
// a namespace-scope constant right behind its table, puts the table on the library's list
struct KernelFamily { const char* name; const KernelInfo* (*at)(int i); };
inline std::vector<KernelFamily>& kernel_families() { static std::vector<KernelFamily> all; return all; }
template <auto& Table>
KernelFamily family(const char* name) {
    return kernel_families().emplace_back(KernelFamily{name, [](int i) -> const KernelInfo* { return i >= 0 && i < (int)std::size(Table) ? &Table[i] : nullptr; }});
}

inline hipError_t opt_in(const KernelFamily& f) {
    for (int i = 0; const KernelInfo* e = f.at(i); ++i)
        if (e->lds_max > 0)
            if (hipError_t r = hipFuncSetAttribute(e->fn, hipFuncAttributeMaxDynamicSharedMemorySize, e->lds_max); r != hipSuccess) return r;
    return hipSuccess;
}
// every table of the library, once per process (kept out of the launch path so that launches are capturable into a hipGraph)
inline hipError_t init_kernel_tables() {
    for (const KernelFamily& f : kernel_families())
        if (hipError_t r = opt_in(f); r != hipSuccess) return r;
    return hipSuccess;
}

}  // namespace dd
