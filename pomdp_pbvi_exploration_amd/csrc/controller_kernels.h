// Finite-state controller evaluation (pbvi_controller_value_iteration): one Jacobi sweep of
//   V'[n][s] = ER[s,a_n] + gamma * sum_o sum_r RTO[s,a_n,o,r] * V[succ[n][o]][rs[s,a_n,r]]
// over all (node, state).  include/pbvi_hip.h has the definition, operation for operation; the products and sums are
// un-fused and in that order, so rows and changes agree bit for bit with pomdp.controller_numpy on finite inputs.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pbvi {

// Nodes one thread of the tiled kernel carries.  The caller orders the nodes of a run by action (stably), so a tile is a
// run of consecutive nodes with one action: one load of an RTO / rs element then serves every node of the tile.
constexpr int CONTROLLER_NODE_TILE = 4;

// One sweep `it` of a run.  Every pointer is device memory.
struct ControllerSweep {
    int S, A, O, R, N;
    const int32_t* rs;                // [A][R][S]
    const double* rto;                // [A][O][R][S]
    const double* er;                 // [A][S]
    const int32_t* node_action;       // [N], every entry in [0, A)
    const int32_t* node_succ;         // [N][O], every entry in [0, N)
    int node_tile;                    // 1: one node per thread, tile t is node t (tile_first is not read);
                                      // CONTROLLER_NODE_TILE: tiles as listed in tile_first
    int tiles;                        // node tiles (N when node_tile = 1)
    const int32_t* tile_first;        // [tiles + 1]: tile t holds nodes [tile_first[t], tile_first[t+1]), between 1 and
                                      // node_tile of them, all with the action of the first
    double gamma, limit;
    int it;
    const double* v_in;               // [N][S]
    double* v_out;                    // [N][S]
    double* changes;                  // [horizon], zeroed before sweep 0: changes[it] = max |v_out - v_in|
};
// k_controller_sweep<NT>: grid = tiles * ceil(S / 256) blocks of 256 threads (the caller keeps that product within int32).
// A sweep behind one that met the limit (changes[it-1] < limit) leaves at once and writes nothing.
hipError_t launch_controller_sweep(const ControllerSweep& cs, hipStream_t st);

}  // namespace pbvi
