// The sweep kernels of the handle-free value-iteration entries (include/pbvi_hip.h has each definition, operation for
// operation):
//   pbvi_mdp_value_iteration         Q'(s,a)  = ER[s,a]   + gamma * sum_r P[s,a,r] * V(rs[s,a,r]),  V' = max_a Q'(., a)
//   pbvi_fib_value_iteration         Q'(s,a)  = ER[s,a]   + gamma * sum_o max_a' sum_r RTO[s,a,o,r] * Q(rs[s,a,r], a')
//   pbvi_controller_value_iteration  V'[n][s] = ER[s,a_n] + gamma * sum_o sum_r RTO[s,a_n,o,r] * V[succ[n][o]][rs[s,a_n,r]]
// Every product and sum is un-fused and in the order of the definition, so rows and changes agree bit for bit with the
// host restatements (pomdp.fib_numpy, pomdp.controller_numpy) on finite inputs.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pbvi {

// What every sweep `it` of a run is given.  Every pointer is device memory; the tables are re-tiled so that with s across
// the lanes every table load is coalesced.
struct SweepArgs {
    int S, A, O, R;
    const int32_t* rs;                // [A][R][S], every entry in [0, S)
    const double* rto;                // [A][O][R][S]
    const double* er;                 // [A][S]
    double gamma, limit;
    int it;
    double* changes;                  // [horizon], zeroed before sweep 0: changes[it] = max |new - old| of sweep it
};
// A sweep behind one that met the limit (changes[it-1] < limit) leaves at once and writes nothing, so the host can enqueue
// sweeps in batches without syncing; the result of the converged sweep stays in place.

// k_vi_sweep: O = 1 and rto is the transition probability [A][R][S].  grid = ceil(S / 256) blocks of 256 threads.
struct ViSweep : SweepArgs {
    const double* v_in;               // [S]
    double* v_out;                    // [S]: max_a rows[a]
    double* rows;                     // [A][S]
};
hipError_t launch_vi_sweep(const ViSweep& vs, hipStream_t st);

// k_fib_sweep<TW, PAIRS>: grid = A * ceil(S / 256) blocks of 256 threads (within int32 as S * A is).
struct FibSweep : SweepArgs {
    const double* q_in;               // [S][A]
    double* q_out;                    // [S][A]
};
hipError_t launch_fib_sweep(const FibSweep& fs, hipStream_t st);

// Nodes one thread of the tiled controller kernel carries.  The caller orders the nodes of a run by action (stably), so a
// tile is a run of consecutive nodes with one action: one load of an RTO / rs element then serves every node of the tile.
constexpr int CONTROLLER_NODE_TILE = 4;

// k_controller_sweep<NT>: grid = tiles * ceil(S / 256) blocks of 256 threads (the caller keeps that product within int32).
struct ControllerSweep : SweepArgs {
    int N;
    const int32_t* node_action;       // [N], every entry in [0, A)
    const int32_t* node_succ;         // [N][O], every entry in [0, N)
    int node_tile;                    // 1: one node per thread, tile t is node t (tile_first is not read);
                                      // CONTROLLER_NODE_TILE: tiles as listed in tile_first
    int tiles;                        // node tiles (N when node_tile = 1)
    const int32_t* tile_first;        // [tiles + 1]: tile t holds nodes [tile_first[t], tile_first[t+1]), between 1 and
                                      // node_tile of them, all with the action of the first
    const double* v_in;               // [N][S]
    double* v_out;                    // [N][S]
};
hipError_t launch_controller_sweep(const ControllerSweep& cs, hipStream_t st);

}  // namespace pbvi
