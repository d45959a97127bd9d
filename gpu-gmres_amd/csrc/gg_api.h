// gg_api.h -- the C ABI's exception boundary (solver.hip, dd.hip, batch.hip,
// cg_batch.hip, bicgstab_batch.hip): an entry point's body between GG_API_BEGIN and GG_API_END
// returns its own code, or the code of what it threw with the text left for
// gg_last_error.
#pragma once

#include <exception>
#include <new>

#include "gg_internal.h"

namespace gg {
inline int fail(const Error &e)
{
    set_error(e.msg);
    return e.code;
}
}  // namespace gg

#define GG_API_BEGIN try {
#define GG_API_END                                                                              \
    }                                                                                           \
    catch (const gg::Error &e) { return gg::fail(e); }                                          \
    catch (const std::bad_alloc &) { return gg::fail({GG_ENOMEM, "host allocation failed"}); } \
    catch (const std::exception &e) { return gg::fail({GG_EINVAL, e.what()}); }
