// ctx_access.h -- what the entry points that live outside icp_context.cpp may know about a so_icp_ctx (the struct itself stays
// private to icp_context.cpp).
#pragma once
#include <string>

#include "../../include/so_icp.h"

namespace soicp {

struct CtxView {
  bool host_only;  // device_id < 0: LocalMap bookkeeping only, every compute entry point fails
};
CtxView ctx_view(const so_icp_ctx* c);
// sets the text so_icp_last_error returns and passes `code` through
int ctx_note(so_icp_ctx* c, int code, const std::string& msg);

}  // namespace soicp
