// ftte_plan.cpp -- the cached callers of the uniform-grid planners: the plan of the ray-following tiles (build_plan) and of the
// cell-fixed bricks (build_brick_plan) is kept in the context for as long as the directions, the grid and what the options resolve
// to stay the same.  The planners themselves read no context (plan_tiles, plan_bricks: ftte_planner.cpp); here the options are
// resolved, the key compared, the counters bumped and a failure turned into the context's error.
#include "ftte_context.h"

namespace ftte {

int build_plan(ftte_ctx *c, int rows, int stack, int ndir, const double *phi, const double *theta, const double *w)
{
    Plan &P = c->plan;
    if (P.valid && P.n == c->n && P.rows == rows && P.slots == c->opt.tile.slots && P.stack == stack && P.box == c->box && same_list(P.phi, phi, ndir) &&
        same_list(P.theta, theta, ndir) && same_list(P.w, w, ndir))
        return FTTE_OK;
    ++c->n_plan_builds;
    c->plan_uploaded = false;
    std::string why;
    const int rc = plan_tiles(TileInputs{c->n, c->box, rows, stack, c->opt.tile.slots, ndir, phi, theta, w}, P, &why);
    return rc ? fail(c, rc, why) : FTTE_OK;
}

int build_brick_plan(ftte_ctx *c, int ndir, const double *phi, const double *theta, const double *w)
{
    BrickPlan &P = c->bplan;
    BrickKey key = c->opt.brick.resolve(c->n, c->nnu, c->emit_mode);
    key.box = c->box;
    if (key.want_dataflow && c->opt.brick.dataflow == 3) { // persistent workgroups, a queue per XCD: needs to know the XCDs
        const int rc = xcc_census(c);
        if (rc) return rc;
        c->opt.brick.persistent(key, c->nnu, c->xcc_count);
    }
    c->opt.brick.visits(key, c->nnu, c->emit_mode, c->opt.launch.plain()); // two passes per visit, where the sweep has the form for it

    if (P.valid && P.key == key && same_list(P.phi, phi, ndir) && same_list(P.theta, theta, ndir) && same_list(P.w, w, ndir)) return FTTE_OK;
    ++c->n_plan_builds;
    const long long id = ++c->brick_plans; // (a new plan: no BrickTables holds it)
    std::string why;
    const int rc = plan_bricks(BrickInputs{key, ndir, phi, theta, w}, P, &why);
    P.id = id;
    return rc ? fail(c, rc, why) : FTTE_OK;
}

} // namespace ftte
