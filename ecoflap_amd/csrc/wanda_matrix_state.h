// wanda_matrix_state.h — K7 matrix mode: the two selection states and the sizes the workspace
// entries of wanda.hip need (sizeof the states, WS_PART_BYTES), and the host interface of
// wanda_matrix.hip.  The kernels and everything else of matrix mode are in wanda_matrix.hip.
#pragma once
#include "wanda_k7.h"

struct MatrixSelState {
    uint32_t hist[3][2048];
    uint32_t resolved[3][2];      // (prefix, remaining rank) after pass 1, 2, 3
    uint32_t pad[58];
};

// Matrix mode runs FEW, LARGE workgroups (1024 threads, 256 over the launch, shared out by size):
// every workgroup merges its LDS histogram into the matrix's global one with one atomic per
// non-empty bin, and those atomics all meet at the memory side — with 1024 workgroups per matrix
// that merge, not the read of W, was the whole cost of a pass (measured: 74 us for a 50 MB ViT-g
// block).  What a pass costs today is mostly fixed: a matrix of 2 M elements takes ~10 us per
// pass like one of 8 M (launch, zeroing + staging LDS, resolving the earlier passes from the
// global histograms, the merge); the streaming itself runs at > 5 TB/s.
#define WM_THREADS 1024
#define WM_WAVES (WM_THREADS / 64)
#define WM_TOTAL_WGS 256     // one workgroup per CU over the whole launch (measured: 128 and 512 both slower)
#define WM_SUB0 4            // interleaved counters per bin in the first pass
#define WM_UNROLL 4
#define WM_SQ_LDS 16384      // columns whose sqrt table is staged in LDS (64 KiB of the CU's 160)

#define WS_SAMPLE_VECS 2048
#define WS_BINS 512
#define WS_CAP 16384                    // list of the threshold bin's elements (LDS of the settling workgroup)
// Matrices of more elements than this keep the three-histogram selection: the bracket holds up to
// ~8.5 % of a matrix (5 sigma of the sample plus a sample bin either side) in 256-512 histogram
// bins, so the threshold's bin of a larger matrix would outgrow the list and every such call
// would end in the one-workgroup fallback.
#define WS_MAX_NUMEL (48ll << 20)
#define WS_PRE 4                        // vectors per thread in registers across the prologue (see below)
#define WS_PART_WORDS (WS_BINS + 8)     // a workgroup's slot: histogram, count below the bracket

struct BracketState {
    uint32_t list_count, ticket, fallback, pad;     // cleared by the counting pass
    uint32_t lo, hi, shift, valid;                  // written by the counting pass
    uint32_t list_idx[WS_CAP];
    uint32_t list_bits[WS_CAP];
};

// the counting pass's slots, one per workgroup of a launch (matrix-mode groups run one after the
// other on the stream and share them)
#define WS_PART_BYTES ((size_t)(WM_TOTAL_WGS + WMAX) * WS_PART_WORDS * sizeof(uint32_t))

// Which matrix-mode items take the sampled bracket (reads ECOFLAP_WANDA_SAMPLED, at every call).
// Decided before the sqrt launch: those items stage sqrt(scaler_row) themselves.
void wanda_matrix_sampled(const ecoflap_wanda_item* items, int n_items, float* const* sq, bool* sampled_item);
// Every item not yet `done`: groups by (dtype, vector form, path), shares out the workgroups,
// launches the three histograms + apply or the sampled bracket + apply.  0 or an error code.
int wanda_matrix_launch(const ecoflap_wanda_item* items, int n_items, float* const* sq,
                        MatrixSelState* const* st, BracketState* const* bst, uint32_t* part,
                        const bool* sampled_item, bool* done, hipStream_t s);
