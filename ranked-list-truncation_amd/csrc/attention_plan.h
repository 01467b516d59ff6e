// The list-axis attention's dispatch plan: which kernel runs each part of a call, which prepare passes precede it, and how the
// forward's `images` and the backward workspace are laid out.  attn_plan() (attention_dispatch.hip) takes the decision ONCE per
// call; the public entry points read it and the family launchers (attention_common.h) are handed its kernel codes - none of them
// decides anything from an environment switch, a shape or a null pointer again.  The plan is the public query struct: kernel,
// prepare, layout codes are the RLT_ATTN_* of include/rlt_hip.h.
#pragma once
#include "common.h"

typedef rlt_attention_plan AttnPlan;

// Pure in (arguments, the calling thread's precision scope, the environment switches read once per process).  have_images: the
// call has a usable `images` buffer (see rlt_list_attention_plan).  The layout fields (images_*, flags_*, delta_bytes, ws_kind,
// ws_extra_bytes, ws_bytes) do not depend on have_images: they are what the workspace queries return.
AttnPlan attn_plan(int S, int B, int H, int HD, float drop_p, bool have_images);
