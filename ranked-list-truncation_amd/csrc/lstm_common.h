// Shared between lstm.hip and lstm6w.hip: the fused input projection of narrow inputs (I <= 3, the reference's score / tf-idf /
// doc2vec features, models/AttnCut.py:8,17) and the internal launchers of the whole-weights recurrences.
#pragma once
#include <stddef.h>
#include "common.h"

struct RltXIn {
    const float* x;            // (S*B, I) position-major, or null: `gates` holds the pre-activations
    const float* w_ih[2];      // (512, I) per direction
    const float* b_ih[2];
    const float* b_hh[2];
    int I;
};

// The recurrence's dispatch plan: which kernel runs the forward and the backward of a call and how many lists a workgroup of it
// owns.  lstm_plan() (lstm.hip) takes the decision ONCE per call; launch_bilstm_fwd, rlt_bilstm_rec_bwd and the launchers below are
// handed its kernel codes (RLT_LSTM_* of include/rlt_hip.h) - none of them reads an environment switch or a batch size again.
// Pure in (B, the calling thread's precision scope, the environment switches read once per process).
typedef struct rlt_bilstm_rec_plan LstmPlan;
LstmPlan lstm_plan(int B);

// lstm6w.hip: bf16x6 recurrences with one wavefront per SIMD; kernel: RLT_LSTM_X6W_SINGLE or RLT_LSTM_X6W_HALVES, lists: the
// plan's lists per workgroup; 0 or a hip error code
int rlt_lstm6w_fwd(int kernel, int lists, float* gates, const float* w_hh_fwd, const float* w_hh_rev, int S, int B, float* h_out, float* c_out,
                   const RltXIn& xi, void* stream);
int rlt_lstm6w_bwd(int kernel, int lists, float* gates, const float* c, const float* w_hh_fwd, const float* w_hh_rev, const float* d_hout, int S, int B,
                   void* stream);
