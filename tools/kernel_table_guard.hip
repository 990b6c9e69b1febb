// Stand-alone host check of csrc/kernel_table.h (no GPU needed): a launch that finds no entry, or asks for more dynamic LDS than its entry is
// opted in to, returns hipErrorInvalidValue before the typed launcher runs, i.e. before anything touches a device.
//     hipcc -std=c++20 --offload-arch=gfx950 -I duodiff_amd/csrc tools/kernel_table_guard.hip -o guard && ./guard
#include "kernel_table.h"

#include <cstdio>

namespace {

struct Args { float* out; int n; };
__global__ void dummy_kernel(const Args a) { if ((int)threadIdx.x < a.n) a.out[threadIdx.x] = 0.f; }

int launches = 0;
void counting_run(dim3, dim3, size_t, hipStream_t, Args) { ++launches; }

int failures = 0;
void expect(bool ok, const char* what) {
    std::printf("%s: %s\n", ok ? "ok" : "FAILED", what);
    failures += !ok;
}

}  // namespace

int main() {
    using namespace dd;
    // an entry as the tables make them (the launcher's parameter is the kernel's own Args) and one whose launcher only counts
    const KernelEntry<Args> table[] = {entry<dummy_kernel>({512, 1}, 256, 96 * 1024), {{{512, 2}, nullptr, 256, 96 * 1024}, counting_run}};
    const Args a{nullptr, 0};
    expect(find(table, 512, 1) == &table[0] && find(table, 512, 2) == &table[1], "find returns the entry of a key");
    expect(find(table, 512, 3) == nullptr && find(table, 256, 1) == nullptr && find(table, 512) == nullptr, "find returns null for a key without an entry");
    expect(launch(find(table, 512, 3), dim3(1), 0, nullptr, a) == hipErrorInvalidValue, "no entry: hipErrorInvalidValue");
    expect(launch(&table[0], dim3(1), 96 * 1024 + 1, nullptr, a) == hipErrorInvalidValue, "one byte over lds_max, real kernel: hipErrorInvalidValue");
    expect(launch(&table[1], dim3(1), 96 * 1024 + 1, nullptr, a) == hipErrorInvalidValue && launches == 0, "one byte over lds_max: refused before the launcher runs");
    expect(launch(&table[1], dim3(1), (size_t)1 << 40, nullptr, a) == hipErrorInvalidValue && launches == 0, "2^40 bytes: refused before the launcher runs");
    (void)launch(&table[1], dim3(1), 96 * 1024, nullptr, a);
    expect(launches == 1, "exactly lds_max: the launcher runs");
    return failures ? 1 : 0;
}
