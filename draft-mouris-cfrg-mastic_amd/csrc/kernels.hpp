// HIP kernels of the batched Mastic aggregator (gfx950): the index of the
// device headers.  The code is in the headers included below, one per subsystem.
//
// Data layout in HBM: every per-report vector is stored as word PLANES,
// plane[w][stride] with stride = reports padded to a multiple of 64, so lane
// r of a wave always touches word r of a plane: all loads/stores coalesce.
// The tree shape (agg_param) is shared by every report of a batch, so all
// control flow below is wave-uniform; only data differs per lane.
//
// Reference mapping (poc/), with the header of each kernel:
//   k_eval_aes     level_kernel.hpp
//                  Vidpf.eval_with_siblings / eval_next / extend / convert
//                  (vidpf.py:213-364) for one tree level, plus the per-parent
//                  payload difference of Mastic.prep_init (mastic.py:267-271)
//                  and the truncated out shares (:311-314)
//   k_node_proof   node_proof.hpp
//                  Vidpf.node_proof (vidpf.py:366-380) for one tree level
//   k_absorb       absorb_kernels.hpp
//                  the one-hot / payload binders' TurboSHAKE absorption
//                  (mastic.py:259-287), streamed level by level
//   k_finalize     finish_kernels.hpp
//                  payload/onehot checks, counter check, eval proof (:277-306)
//   k_flp_rand     finish_kernels.hpp
//                  query rand, helper proof share, joint rand (:437-510)
//   k_flp_query    finish_kernels.hpp
//                  FlpBBCGGI19.query (:250-256)
//   k_fold         fold_kernels.hpp
//                  agg_update / merge over reports (:379-397)
//   k_decide       decide_kernels.hpp
//                  prep_shares_to_prep (:320-362)
//   k_decide_peer  decide_kernels.hpp
//                  prep_shares_to_prep + one aggregator's prep_next (:320-377),
//                  its own result planes against the peer's wire prep shares
// Without a counterpart in the reference: the wire unpacking and key setup
// (unpack_kernels.hpp), the prefix states (planes.hpp), the convert streams'
// buffering (conv_stream.hpp).  The client's k_shard is shard.hpp's, outside
// this index.
#pragma once
#include "planes.hpp"
#include "unpack_kernels.hpp"
#include "conv_stream.hpp"
#include "node_proof.hpp"
#include "level_kernel.hpp"
#include "absorb_kernels.hpp"
#include "finish_kernels.hpp"
#include "fold_kernels.hpp"
#include "decide_kernels.hpp"
