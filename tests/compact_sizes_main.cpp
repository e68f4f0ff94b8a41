// Stand-alone check (its own main, no GPU work, not loaded into Python) of the workspace sizes that are built on compact_offsets_bytes
// (csrc/compact.h): the size functions of scene.hip, voxel.hip, tsdf.hip and match.hip at boundary sizes against the formulas those
// files held before the header existed, written out here.  Built with the host-side address and
// undefined-behaviour sanitizers by tests/test_compact_sizes_cpu.py.
#include "compact.h"
#include "scene.h"

#include <cstdio>
#include <cstdlib>

using a3r::align_up;

// scene.hip's way to the aligner handle (align.hip, not linked here); the size functions never get there
int a3r::align_scene_view(a3r_align_t, hipStream_t, SceneView*, const char*) { return A3R_EINVAL; }

static int failures = 0;

static void expect(const char* what, long long a, long long b, long long c, size_t got, size_t want) {
    if (got == want) return;
    std::printf("%s(%lld, %lld, %lld) = %zu, the earlier formula gives %zu\n", what, a, b, c, got, want);
    failures++;
}

static size_t offsets_before(size_t T) { return align_up((T + 1) * sizeof(int), 256); }
static size_t chunks_of(long long n) { return (size_t)((n + 1023) / 1024); }        // every family uses chunks of 1024 items

int main() {
    const long long top = (1ll << 31) - 1;
    for (long long T : {0ll, 1ll, 1023ll, 1024ll, 1025ll, 1ll << 21, top})
        expect("compact_offsets_bytes", T, 0, 0, a3r::compact_offsets_bytes((size_t)T), offsets_before((size_t)T));

    // scene.hip: offsets [N * nchunks + 1]; mesh: vertex offsets | face offsets [4 T + 1] | rank map [N, P]
    for (int N : {1, 3, 64})
        for (int P : {1, 1023, 1024, 1025, 1 << 20, 1 << 30}) {
            const size_t T = (size_t)N * chunks_of(P);
            expect("a3r_align_scene_workspace_bytes", N, P, 0, a3r_align_scene_workspace_bytes(N, P), offsets_before(T));
            expect("a3r_align_scene_mesh_workspace_bytes", N, P, 0, a3r_align_scene_mesh_workspace_bytes(N, P),
                   offsets_before(T) + align_up((4 * T + 1) * sizeof(int), 256) + align_up((size_t)N * P * sizeof(int), 256));
        }
    expect("a3r_align_scene_workspace_bytes", 0, 5, 0, a3r_align_scene_workspace_bytes(0, 5), 0);
    expect("a3r_align_scene_mesh_workspace_bytes", 5, 0, 0, a3r_align_scene_mesh_workspace_bytes(5, 0), 0);

    // voxel.hip: head | offsets [nchunks + 1] | slot [M] | keys, best [slots] | count [slots] | sums [slots, 6] (mean)
    for (long long M : {0ll, 1ll, 1024ll, 1025ll, 1024ll * 1024 + 1025, top})
        for (int reduce : {A3R_VOXEL_BEST, A3R_VOXEL_MEAN}) {
            size_t S = 1;
            while ((long long)S < 2 * M && S < ((size_t)1 << 31)) S <<= 1;
            const size_t want = 256 + offsets_before(chunks_of(M)) + align_up((size_t)M * 4, 256) + 2 * align_up(S * 8, 256) + align_up(S * 4, 256) +
                                (reduce == A3R_VOXEL_MEAN ? align_up(S * 48, 256) : 0);
            expect("a3r_voxel_workspace_bytes", M, 0, reduce, a3r_voxel_workspace_bytes(M, 0, reduce), want);
        }
    expect("a3r_voxel_workspace_bytes", top + 1, 0, 0, a3r_voxel_workspace_bytes(top + 1, 0, A3R_VOXEL_BEST), 0);

    // tsdf.hip: vertex offsets | quad offsets [nchunks + 1] | rank map [nvox]; at most 2^31 / 6 voxels
    const int most = (int)((1ll << 31) / 6);
    for (int nx : {1, 1024, 1025, most}) {
        const size_t nvox = (size_t)nx;
        expect("a3r_tsdf_mesh_workspace_bytes", nx, 1, 1, a3r_tsdf_mesh_workspace_bytes(nx, 1, 1),
               2 * offsets_before(chunks_of(nx)) + align_up(nvox * sizeof(int), 256));
    }
    expect("a3r_tsdf_mesh_workspace_bytes", 0, 1, 1, a3r_tsdf_mesh_workspace_bytes(0, 1, 1), 0);
    expect("a3r_tsdf_mesh_workspace_bytes", most + 1, 1, 1, a3r_tsdf_mesh_workspace_bytes(most + 1, 1, 1), 0);

    // match.hip with one data range forced: search partials (the larger direction) | nn1 [n1] | offsets [blocks + 1]
    for (long long n1 : {1ll, 1000ll})
        for (long long n2 : {1ll, 1024ll, 1025ll, 1024ll * 1024 + 1025, top}) {
            const size_t a = align_up((size_t)n2 * 8, 256) + align_up((size_t)n2 * 4, 256), b = align_up((size_t)n1 * 8, 256) + align_up((size_t)n1 * 4, 256);
            expect("a3r_match_workspace_bytes", n1, n2, 1, a3r_match_workspace_bytes(n1, n2, 1),
                   (a > b ? a : b) + align_up((size_t)n1 * 4, 256) + offsets_before(chunks_of(n2)));
        }
    expect("a3r_match_workspace_bytes", 0, 7, 1, a3r_match_workspace_bytes(0, 7, 1), 0);
    expect("a3r_match_workspace_bytes", 7, top + 1, 1, a3r_match_workspace_bytes(7, top + 1, 1), 0);

    if (failures == 0) std::printf("ok\n");
    return failures == 0 ? EXIT_SUCCESS : EXIT_FAILURE;
}
