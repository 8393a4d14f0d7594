// ctx_access.h -- what the entry points that live outside icp_context.cpp may know about a so_icp_ctx (the struct itself stays
// private to icp_context.cpp).
#pragma once
#include <hip/hip_runtime_api.h>

#include <memory>
#include <string>

#include "../../include/so_icp.h"

namespace soicp {

struct CtxView {
  bool host_only;  // device_id < 0: LocalMap bookkeeping only, every compute entry point fails
};
CtxView ctx_view(const so_icp_ctx* c);
// sets the text so_icp_last_error returns and passes `code` through
int ctx_note(so_icp_ctx* c, int code, const std::string& msg);

// what a device entry point outside icp_context.cpp needs (device contexts only)
struct CtxDevice {
  int device_id;
  hipStream_t stream;  // the context's queue: work on a caller's device buffers
  hipStream_t aux;     // the queue of the host-in / host-out steps around Localization() (pre-filter, de-skew)
  // state of such an entry point, owned by the context: created by its user, released (before the queues) when the context goes
  std::shared_ptr<void>* ext_features;
};
CtxDevice ctx_device(so_icp_ctx* c);

}  // namespace soicp
