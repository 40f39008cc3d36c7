// The tree tensors of the torch ops as the C ABI's tree (include/mzba.h mzba_tree_step): the one validation behind
// mcts_root_ / _select_ / _backup_ / _results_ (torch_ops.cpp) and prediction_tree_ (net_ops.cpp).
#pragma once
#include <ATen/ATen.h>

#include "../../include/mzba.h"

namespace {

void check_dev(const at::Tensor& t, const char* name, at::ScalarType st) {
  TORCH_CHECK(t.is_cuda(), "mz: ", name, " must be a device tensor");
  TORCH_CHECK(t.scalar_type() == st, "mz: ", name, " has dtype ", t.scalar_type(), ", expected ", st);
  TORCH_CHECK(t.is_contiguous(), "mz: ", name, " must be contiguous");
}

// B trees of S simulations: nodes and path of exactly that size, the per-env buffers at least B entries, the tables
// at least S + 1. sim, gamma and r are left zero for the caller.
mzba_tree_step tree_step_of(int64_t B, const at::Tensor& nodes, const at::Tensor& root_sum, const at::Tensor& calls,
                            const at::Tensor& leaf_parent, const at::Tensor& leaf_action, const at::Tensor& depth,
                            const at::Tensor& path, const at::Tensor& sqrt_tab, const at::Tensor& c_tab, int64_t S,
                            int64_t env_offset, int64_t search_id, int64_t seed, const c10::optional<at::Tensor>& ctx) {
  check_dev(nodes, "nodes", at::kByte);
  check_dev(root_sum, "root_sum", at::kFloat);
  check_dev(calls, "calls", at::kInt);
  check_dev(leaf_parent, "leaf_parent", at::kInt);
  check_dev(leaf_action, "leaf_action", at::kInt);
  check_dev(depth, "depth", at::kInt);
  check_dev(path, "path", at::kInt);
  check_dev(sqrt_tab, "sqrt_tab", at::kFloat);
  check_dev(c_tab, "c_tab", at::kFloat);
  TORCH_CHECK(S > 0 && B > 0, "mz: empty tree batch");
  TORCH_CHECK(nodes.numel() == B * (S + 1) * mzba_mcts_node_bytes() && path.numel() == B * (S + 1) &&
                  root_sum.numel() >= B && calls.numel() >= B && leaf_parent.numel() >= B && leaf_action.numel() >= B &&
                  depth.numel() >= B && sqrt_tab.numel() >= S + 1 && c_tab.numel() >= S + 1,
              "mz: tree buffer sizes do not match B = ", B, ", S = ", S);
  return mzba_tree_step{nodes.data_ptr(), root_sum.data_ptr<float>(),
                        reinterpret_cast<uint32_t*>(calls.data_ptr<int32_t>()), leaf_parent.data_ptr<int32_t>(),
                        leaf_action.data_ptr<int32_t>(), depth.data_ptr<int32_t>(), path.data_ptr<int32_t>(),
                        sqrt_tab.data_ptr<float>(), c_tab.data_ptr<float>(), (int)B, (int)S, (int)env_offset,
                        (int)search_id, (uint64_t)seed,
                        ctx.has_value() && ctx->defined() ? ctx->data_ptr<int32_t>() : nullptr, 0, 0.f, nullptr};
}

}  // namespace
