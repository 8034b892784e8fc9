// route.cpp -- glrt_launch_route (include/glrt_host.h): the route statement (route_statement.h) behind the C ABI.
#include <cstdio>

#include "glrt_host.h"
#include "route_statement.h"

int glrt_launch_route(const glrt_route_state *state, int kind, glrt_route *route_out, char *msg, size_t cap) {
    if (msg && cap) msg[0] = 0;
    if (!state || !route_out || kind < 0 || kind >= glrt_detail::kRouteKinds) return GLRT_HOST_EINDEX;
    const glrt_route_state &s = *state;
    const glrt_detail::RouteState rs{s.variant,       s.ext_flags,     s.n_spheres,      s.n_tex,         s.n_vine,          s.have_volume != 0, s.have_maps != 0,
                                     s.have_cut != 0, s.have_emit != 0, s.have_env != 0, s.vol_switch != 0, s.tex_switch != 0, s.max_depth,        s.n_samples};
    const glrt_detail::Route r = glrt_detail::launch_route(rs, (glrt_detail::RouteKind)kind);
    *route_out = glrt_route{};
    if (!r.refusal.empty()) {
        if (msg && cap) std::snprintf(msg, cap, "%s", r.refusal.c_str());
        return GLRT_HOST_EINVAL;
    }
    route_out->family = route_out->variant_last = r.family;
    route_out->fallback_last = r.fallback;
    route_out->fallback_counts = r.fallback_counts;
    route_out->form = r.form;
    std::snprintf(route_out->kernel, sizeof route_out->kernel, "%s", r.kernel);
    return GLRT_HOST_OK;
}
