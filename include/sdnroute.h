/*
 * sdnroute.h -- C ABI of the MI355X route engine (libsdnroute.so).
 *
 * Drop-in boundary for the route hot path of keichi/sdn-mpi-router:
 * the Python TopologyDB (reference sdnmpi/util/topology_db.py:8) keeps its
 * API and dict state; its route computation is replaced by per-source /
 * per-destination tables computed by the HIP kernels behind these entry
 * points.  The reference has no FFI of its own (it is pure Python); these
 * are the entry points a ctypes binding of that class binds (INTEGRATION.md
 * shows the binding, sdn-mpi-router_amd/sdnmpi_amd/_native.py is ours).
 *
 * Conventions
 *  - Every call returns SDNR_OK (0) or a negative errno-style code; the
 *    message of the last failure on the calling thread is sdnr_last_error().
 *  - Graph = dense CSR, vertex i = i-th smallest dpid, each row sorted
 *    strictly ascending (== sorted(self.links[dpid].keys()),
 *    topology_db.py:76), port[e] = links[u][v].src.port_no (:130).
 *  - Tables are row-major [n_rows][V] int32 (dist: uint16); the caller owns
 *    every buffer.  Without SDNR_DEVICE_PTRS they are host buffers and the
 *    call is synchronous; with it they are device buffers on the context's
 *    device and the call is asynchronous on the context's stream.
 *  - Unreachable entries are SDNR_UNREACHED (-1) / SDNR_DIST_INF (0xFFFF).
 *  - A context is not re-entrant (the reference calls TopologyDB from
 *    Ryu's single OS thread); distinct contexts are independent.
 */
#ifndef SDNROUTE_H
#define SDNROUTE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDNR_ABI_VERSION 1

#define SDNR_OK          0
#define SDNR_ERR_INVAL (-22)  /* EINVAL: bad argument / malformed CSR      */
#define SDNR_ERR_NOMEM (-12)  /* ENOMEM: device or host allocation failed  */
#define SDNR_ERR_NODEV (-19)  /* ENODEV: no such HIP device                */
#define SDNR_ERR_STATE (-77)  /* EBADFD: no graph uploaded to the context  */
#define SDNR_ERR_HIP   (-5)   /* EIO:    HIP runtime error                 */

#define SDNR_DEVICE_PTRS 0x1u /* table/source pointers are device pointers */
#define SDNR_TIMING      0x2u /* time the main kernel (sdnr_last_kernel_ms) */
#define SDNR_SAME_TABLES 0x4u /* route expansion: the parent / port tables are the
                                 ones (same pointers, same contents) of the
                                 previous expansion on this context -- its
                                 derived walk tables are reused */
#define SDNR_LOADS_TO_ROOT 0x8u /* sdnr_link_loads: rows are per-destination
                                 next-hop rows (edges point toward the root) */
#define SDNR_LOADS_SPLIT_HOP 0x10u /* sdnr_ecmp_link_loads: every switch splits
                                 evenly over its next hops (default: evenly
                                 over the pair's shortest routes) */
#define SDNR_LFA_LINK_ONLY 0x20u /* sdnr_lfa_tables: link-protecting alternates
                                 only -- node protection is neither evaluated
                                 nor reported, and no neighbour-pair scratch
                                 is needed */

#define SDNR_UNREACHED (-1)
#define SDNR_DIST_INF  0xFFFFu
#define SDNR_TREE_NONE 0xFFFFFFFFu
#define SDNR_COST_INF 0xFFFFFFFFu /* sdnr_cost_tables: no route */

typedef struct sdnr_ctx sdnr_ctx;

/* ABI version of the loaded library (== SDNR_ABI_VERSION it was built with) */
int sdnr_abi_version(void);

/* Build identity: the SHA-256 (64 hex digits) of the sources, headers and
 * compile flags the library was built from ("unversioned" for a build made
 * without it).  The Python loader refuses a library whose id is not the
 * tree's (sdn-mpi-router_amd/sdnmpi_amd/_buildinfo.py). */
const char *sdnr_build_id(void);

/* Message of the last failing call on this thread ("" if none). */
const char *sdnr_last_error(void);

/* Number of visible HIP devices. */
int sdnr_device_count(int *count);

/* Create / destroy a context bound to HIP device `device`.  The context owns
 * the uploaded graph, scratch memory and a HIP stream.
 * Replaces the state of TopologyDB.__init__ (topology_db.py:9-18). */
int sdnr_create(int device, sdnr_ctx **out);
int sdnr_destroy(sdnr_ctx *ctx);

/* A context over several devices of one node (the controller's single
 * TopologyDB, reference sdnmpi/topology.py:67, driving all of them; SURVEY.md
 * 8(e)).  devices[0] is the primary: device-pointer buffers live there and
 * asynchronous work is ordered on its stream.  Every device holds a copy of
 * the uploaded graph; sdnr_dfs_tables, sdnr_dfs_tables_packed and
 * sdnr_shortest_tables split their ids into ndev contiguous shards, one per
 * device (each with its own stream), and assemble the rows in the caller's
 * tables -- host buffers by one device-to-host copy per shard, primary-device
 * buffers by peer copies over xGMI (fork/join events on the primary stream).
 * The other entry points run on the primary device.  A device may be listed
 * more than once (several shards on one device).  Destroy with sdnr_destroy. */
int sdnr_create_multi(const int *devices, int ndev, sdnr_ctx **out);

/* Devices of a context in shard order: *n = their number; the first
 * min(*n, cap) are written to devices (may be NULL). */
int sdnr_device_list(const sdnr_ctx *ctx, int *devices, int cap, int *n);

/* Run subsequent asynchronous work on `hip_stream` (a hipStream_t of the
 * context's device, e.g. torch.cuda.current_stream().cuda_stream); NULL
 * restores the context's own stream. */
int sdnr_set_stream(sdnr_ctx *ctx, void *hip_stream);

/* Wait for all work queued on the context's stream.  Also reports (as
 * SDNR_ERR_HIP) a kernel whose bounded internal wait ran out -- the
 * kernels never spin unboundedly; that only happens on a bug. */
int sdnr_synchronize(sdnr_ctx *ctx);

/* Upload the switch graph (host buffers).  Replaces the graph state that
 * add_switch/add_link/delete_* maintain (topology_db.py:14-42); the Python
 * side re-exports and re-uploads whenever that state changes.  Validates
 * the CSR (monotone row_ptr, rows strictly ascending, 0 <= col < V). */
int sdnr_graph_upload(sdnr_ctx *ctx, int32_t V, int32_t E,
                      const int32_t *row_ptr, const int32_t *col,
                      const int32_t *port);

/* V, E and maximum out-degree of the uploaded graph (NULL fields skipped). */
int sdnr_graph_info(const sdnr_ctx *ctx, int32_t *V, int32_t *E,
                    int32_t *max_degree);

/* Twin classes of the uploaded graph: rep[v] (V entries, host buffer) = the
 * smallest vertex with the same out-row and the same in-row as v (v itself
 * when there is none, or when v's row holds a self-loop).  The default-route
 * rows of a class differ in a few entries only, so a large sdnr_dfs_tables*
 * batch searches one member per class and derives the other rows. */
int sdnr_graph_twin_reps(sdnr_ctx *ctx, int32_t *rep);

/* Default route, find_route(src, dst) (multiple=False) -> _find_route_dfs
 * (topology_db.py:59-84, called from :181-188), batched over all
 * destinations: for every source src[i] the tree of first pushes of one full
 * LIFO traversal.  Row i of each table (V entries):
 *   parent[i*V+v]  vertex whose pop first pushed v (src[i] for v == src[i]),
 *   port[i*V+v]    links[parent][v].src.port_no (-1 for the root),
 *   hops[i*V+v]    tree depth (0 for the root); hops may be NULL.
 * The route src -> d is the tree path; it equals the reference's route for
 * every d, bit for bit (ports included). */
int sdnr_dfs_tables(sdnr_ctx *ctx, const int32_t *src, int32_t nsrc,
                    int32_t *parent, int32_t *port, int32_t *hops,
                    uint32_t flags);

/* The same default-route trees in the packed layout (4 bytes per entry
 * instead of 8, half the HBM writes, device-to-host copy and all-gather
 * volume):
 *   tree[i*V+v] = parent | port << 16   (parent, port as in sdnr_dfs_tables;
 *                                         port 0xFFFF for the root),
 *   tree[i*V+v] = 0xFFFFFFFF            v unreachable (SDNR_TREE_NONE).
 * Needs V <= 65535 and every port in [0, 0xFFFE] -- OpenFlow 1.0 port
 * numbers are 16-bit (ofp_phy_port.port_no) -- else SDNR_ERR_INVAL. */
int sdnr_dfs_tables_packed(sdnr_ctx *ctx, const int32_t *src, int32_t nsrc,
                           uint32_t *tree, uint32_t flags);

/* The same default-route trees for any fabric size (4 bytes per entry; the
 * packed layout above needs V <= 65535):
 *   tree[i*V+v] = parent | slot << 26   slot: position of v in parent's
 *                                         ascending neighbour list (links[
 *                                         parent] sorted by dpid, the CSR row);
 *                                         the port is that link's src.port_no;
 *                                         slot 63 for the root,
 *   tree[i*V+v] = 0xFFFFFFFF            v unreachable (SDNR_TREE_NONE).
 * The table pass stores one word per vertex and looks no port up.  Needs
 * V < 2^26 and every switch with <= 63 links, else SDNR_ERR_INVAL. */
int sdnr_dfs_tables_slots(sdnr_ctx *ctx, const int32_t *src, int32_t nsrc,
                          uint32_t *tree, uint32_t flags);

/* Pack n entries of int32 default-route tables (sdnr_dfs_tables' parent /
 * port) into the 4-byte layouts above: layout SDNR_TREE_PORT16 = parent |
 * port << 16 (sdnr_dfs_tables_packed), SDNR_TREE_SLOT = parent | slot << 26
 * (sdnr_dfs_tables_slots; the slot is found in the uploaded CSR).  Device
 * pointers only (flags must hold SDNR_DEVICE_PTRS); asynchronous on the
 * context stream.  The route cache of the Python TopologyDB keeps its rows
 * in these layouts (a third of the int32 tables' bytes). */
#define SDNR_TREE_INT32  0   /* int32 parents (sdnr_dfs_rows_affected, sdnr_link_loads) */
#define SDNR_TREE_PORT16 1
#define SDNR_TREE_SLOT   2
int sdnr_tree_pack(sdnr_ctx *ctx, const int32_t *parent, const int32_t *port,
                   int64_t n, uint32_t *tree, int32_t layout, uint32_t flags);

/* Default-route trees straight in a 4-byte layout (SDNR_TREE_PORT16 as
 * sdnr_dfs_tables_packed, SDNR_TREE_SLOT as sdnr_dfs_tables_slots) plus the
 * tree depth -- the rows the Python TopologyDB's route cache keeps (the
 * route lengths of _route_to_fdb, topology_db.py:127-138, and the
 * incremental row tests need the depth):
 *   depth[i*V+v]  hops src[i] -> v; depth_bytes 2: u16, 0xFFFF unreachable
 *                 (needs V <= 65535), 4: int32, -1 unreachable; NULL: none.
 * The same kernels as the benched packed / slot tables, with no int32
 * intermediate. */
int sdnr_dfs_tables_tree(sdnr_ctx *ctx, const int32_t *src, int32_t nsrc,
                         uint32_t *tree, void *depth, int32_t layout,
                         int32_t depth_bytes, uint32_t flags);

/* Incremental recompute on link events: EventLinkAdd /
 * EventLinkDelete -> TopologyDB.add_link / delete_link (reference
 * sdnmpi/topology.py:192-198, sdnmpi/util/topology_db.py:30-42).  Which
 * cached default-route rows a set of link changes alters, decided from the
 * rows themselves: the tree words (layout SDNR_TREE_PORT16 / SDNR_TREE_SLOT
 * as sdnr_dfs_tables_tree writes them, or SDNR_TREE_INT32: int32 parents)
 * and depths (depth_bytes 2: u16, 0xFFFF unreached; 4: int32, -1) of
 * [nrows][V] rows; row_src[r] = the source of row r (-1: a free row, never
 * flagged).  links = (u, v) dense-id pairs: the first nremoved removed or
 * re-ported links, then nadded added links (ids against the CURRENT graph's
 * vertex set, which must equal the rows').  affected[r] = 1 iff the row
 * changes (exact for one link change, a superset for several):
 *   removed / re-ported (u, v): parent[v] == u;
 *   added (u, v): u reached and v unreached, or v pushed in a pop after u's
 *   (preorder, children in descending id order: the two root paths decide).
 * Device pointers only (flags must hold SDNR_DEVICE_PTRS); asynchronous on
 * the context stream; a row that is not a tree is reported by
 * sdnr_synchronize as SDNR_ERR_INVAL. */
int sdnr_dfs_rows_affected(sdnr_ctx *ctx, const uint32_t *tree, const void *depth,
                           int32_t layout, int32_t depth_bytes, int32_t nrows,
                           const int32_t *row_src, const int32_t *links,
                           int32_t nremoved, int32_t nadded, uint8_t *affected,
                           uint32_t flags);

/* Shortest routes, find_route(src, dst, multiple=True) -> _find_routes_bfs
 * (topology_db.py:86-122, called from :168-180), as per-destination tables:
 * for every destination dst[i] and every vertex x
 *   dist[i*V+x]     hop distance x -> dst[i] (SDNR_DIST_INF if none),
 *   nh[i*V+x]       smallest out-neighbour n with dist(n) == dist(x) - 1
 *                   (-1 for x == dst[i] or unreachable),
 *   nh_port[i*V+x]  links[x][nh].src.port_no.
 * Following nh from x gives routes[0] (the lexicographically smallest
 * shortest path); the shortest-path DAG in dist gives the whole ECMP set in
 * the reference's order.  nh / nh_port may be NULL (distances only).
 * A u16 distance holds at most 65,534 hops: the level loops stop there, and a
 * vertex farther from dst[i] reads SDNR_DIST_INF and nh -1, as an unreachable
 * one does (only a graph of more than 65,535 vertices can hold one). */
int sdnr_shortest_tables(sdnr_ctx *ctx, const int32_t *dst, int32_t ndst,
                         uint16_t *dist, int32_t *nh, int32_t *nh_port,
                         uint32_t flags);

/* Per-link costs of the uploaded graph (OSPF / IS-IS style metrics: cost a hot
 * link up, cost a link out for maintenance, prefer the fast links): cost[e] is
 * the cost of the e-th directed link in the uploaded CSR's edge order, E
 * entries in a HOST buffer, copied to the context's primary device.  Checked
 * on the host: every cost >= 1 (a zero would allow cost-neutral cycles) and,
 * with cmax = the largest, cmax * (V - 1) < 0xFFFFFFFF, so no path sum reaches
 * SDNR_COST_INF; else SDNR_ERR_INVAL and the costs in force stay.  NULL clears
 * the costs, and so does sdnr_graph_upload (the edge order changes).  Only
 * sdnr_cost_tables reads them: every other entry point counts hops as before. */
int sdnr_graph_costs(sdnr_ctx *ctx, const uint32_t *cost);

/* Least-cost routes under the uploaded link costs, as per-destination tables
 * (the weighted counterpart of sdnr_shortest_tables): for every destination
 * dst[i] and every vertex x
 *   pcost[i*V+x]    least sum of link costs over the paths x -> dst[i] (0 at
 *                   dst[i], SDNR_COST_INF if there is none),
 *   nh[i*V+x]       smallest out-neighbour n with cost(x -> n) + pcost(n) ==
 *                   pcost(x) (-1 for x == dst[i] or unreachable),
 *   nh_port[i*V+x]  links[x][nh].src.port_no.
 * Following nh from x gives the lexicographically smallest least-cost route
 * (sdnr_shortest_tables' tie rule); costs are positive, so an nh row is an
 * in-tree toward dst[i] and sdnr_link_loads with SDNR_LOADS_TO_ROOT takes it
 * as it is.  With every cost 1 the tables equal sdnr_shortest_tables' (dist
 * widened to u32, SDNR_DIST_INF -> SDNR_COST_INF).  nh and nh_port go together
 * and may both be NULL (costs only).  Everything is integer and bit-exact.
 * Host buffers: synchronous; SDNR_DEVICE_PTRS: asynchronous on the context's
 * stream; SDNR_TIMING as in sdnr_shortest_tables.  Without uploaded costs:
 * SDNR_ERR_STATE.  A destination outside [0, V) is handled as
 * sdnr_shortest_tables handles it: SDNR_ERR_INVAL for host buffers (the ids
 * are checked before anything runs), an empty row (SDNR_COST_INF / -1) for
 * device ids.  One launch (pull Bellman-Ford sweeps to the fixed point, at
 * most V of them; a run that needed more is reported by sdnr_synchronize as
 * SDNR_ERR_INVAL -- costs the upload check would have refused); on a
 * multi-device context it runs on the primary device. */
int sdnr_cost_tables(sdnr_ctx *ctx, const int32_t *dst, int32_t ndst,
                     uint32_t *pcost, int32_t *nh, int32_t *nh_port,
                     uint32_t flags);

/* All-pairs hop distances by min-plus squaring (D <- min(D, D (x) D) until
 * stable) for small dense graphs: dist[i*V+j] = hops i -> j (SDNR_DIST_INF
 * if none).
 * V <= 16384. */
int sdnr_apsp(sdnr_ctx *ctx, uint16_t *dist, uint32_t flags);

/* ECMP sets of find_route(src, dst, multiple=True) (_find_routes_bfs,
 * topology_db.py:86-122: every shortest route, lexicographic dpid order),
 * counted and unranked instead of enumerated.  dist = sdnr_shortest_tables
 * rows ([ndst][V], hops toward each destination).
 * sdnr_ecmp_counts: paths[i*V+x] = number of shortest x -> dst_i routes
 *   (saturating at UINT64_MAX; 1 at the destination, 0 if unreachable).
 * sdnr_ecmp_routes: route k = the ranks[k]-th (0-based, lexicographic) shortest
 *   route from srcs[k] to the destination of row rows[k], as dense vertex ids
 *   src..dst in route_vertices[k*max_len ...], padded with -1; a row of -1
 *   if the rank is out of range or the route is longer than max_len. */
int sdnr_ecmp_counts(sdnr_ctx *ctx, const uint16_t *dist, int32_t ndst,
                     uint64_t *paths, uint32_t flags);
int sdnr_ecmp_routes(sdnr_ctx *ctx, const uint16_t *dist, const uint64_t *paths,
                     int32_t ndst, const int32_t *rows, const int32_t *srcs,
                     const uint64_t *ranks, int32_t nroutes, int32_t max_len,
                     int32_t *route_vertices, uint32_t flags);

/* Flow entries of many host pairs from default-route tables (the OFPFlowMods
 * Router._add_flows_for_path installs, reference sdnmpi/router.py:83-104,
 * for the fdb _route_to_fdb builds, sdnmpi/util/topology_db.py:127-138).
 * Tables: row-major [nrows][V] as returned by sdnr_dfs_tables (hops needed
 * for the sizes).  Pair i is (row rows[i] = its source's tree, destination
 * switch dsts[i], last_port[i] = the destination host's port or OFPP_LOCAL).
 *
 * sdnr_route_offsets: offsets[0..npairs] (int64), offsets[i+1]-offsets[i] =
 *   entries of pair i = hops + 1 (0 if unreachable); offsets[npairs] = total.
 * sdnr_route_expand: for pair i, entries offsets[i]..offsets[i+1]-1 in path
 *   order: hop_switch[j] = dense switch id, hop_port[j] = its out port; the
 *   last entry is (dsts[i], last_port[i]).  Bit-identical to find_route's
 *   fdb with switch ids mapped to dpids.
 * nrows is required in both modes (the expansion builds ancestor
 * tables of the nrows trees).  Host buffers: the tables are staged per call
 * (nrows * V entries each). */
int sdnr_route_offsets(sdnr_ctx *ctx, const int32_t *hops, int32_t nrows,
                       const int32_t *rows, const int32_t *dsts, int32_t npairs,
                       int64_t *offsets, uint32_t flags);
int sdnr_route_expand(sdnr_ctx *ctx, const int32_t *parent, const int32_t *port,
                      int32_t nrows, const int32_t *rows, const int32_t *dsts,
                      const int32_t *last_port, int32_t npairs,
                      const int64_t *offsets, int32_t *hop_switch,
                      int32_t *hop_port, uint32_t flags);

/* Replaces, like sdnr_route_expand, _route_to_fdb for many pairs
 * (sdnmpi/util/topology_db.py:127-138; the entries Router._add_flows_for_path
 * installs, sdnmpi/router.py:83-104).
 * The same entries as ONE u32 word each, switch | out_port << 16 (the
 * packed tree word's layout: a dense switch id and a 16-bit OpenFlow 1.0
 * port, OFPP_LOCAL = 0xfffe included) -- half the bytes of the two int32
 * arrays.  Needs V <= 65535 and 16-bit link ports (else SDNR_ERR_INVAL);
 * a last (host) port outside [0, 0xfffe] fails the call (sdnr_synchronize
 * reports SDNR_ERR_INVAL; 0xffff is the word's "no port", as in the packed
 * tree), so callers with such ports use sdnr_route_expand (the drop-in does).  Device
 * pointers only (flags must hold SDNR_DEVICE_PTRS). */
int sdnr_route_expand_packed(sdnr_ctx *ctx, const int32_t *parent, const int32_t *port,
                             int32_t nrows, const int32_t *rows, const int32_t *dsts,
                             const int32_t *last_port, int32_t npairs, const int64_t *offsets,
                             uint32_t *entries, uint32_t flags);

/* Per-link traffic loads of a routed traffic matrix: how much of a demand
 * crosses each link when every pair takes the controller's route -- what the
 * flow entries of Router._add_flows_for_path (reference sdnmpi/router.py:
 * 83-104, one entry per switch of the route) make the ports carry, and what
 * the real controller observes per port in sdnmpi/monitor.py.  No entry is
 * built: per tree row the load of link parent(v) -> v is the demand destined
 * into v's subtree (ancestor doubling, O(V log depth) per row whatever the
 * number of pairs).
 *   tree      [nrows][V] rows: default-route trees in layout SDNR_TREE_INT32
 *             (int32 parents, sdnr_dfs_tables), SDNR_TREE_PORT16 or
 *             SDNR_TREE_SLOT (sdnr_dfs_tables_tree), row r = one source's tree;
 *   pair_off  [nrows + 1] int64: the pairs of row r are dsts[pair_off[r] ..
 *             pair_off[r+1]) (destination switches, dense ids) with weight[]
 *             (u64, e.g. bytes) at the same indices; weight NULL: all 1;
 *   load      [E] u64 in the uploaded CSR's edge order.  The call ADDS into
 *             load (the caller zeroes it; row chunks of one batch sum up).
 * Per row, load[e(parent(v) -> v)] += sum of the weights of the row's pairs
 * whose destination lies in the subtree of v.  Repeated pairs add; a
 * destination outside [0, V) or unreached in its row contributes nothing;
 * sums are u64 and wrap (bit-exact, order-independent).
 * With SDNR_LOADS_TO_ROOT the rows are per-destination next-hop rows
 * (sdnr_shortest_tables' nh, layout SDNR_TREE_INT32 only; root and unreached
 * vertices hold -1), dsts[] name the flows' SOURCE switches and the link is
 * v -> nh[v]: the loads of routes[0] of find_route(multiple=True).
 * A vertex has no ancestor when its int32 parent is < 0 or itself.
 * Device pointers only (flags must hold SDNR_DEVICE_PTRS); asynchronous on
 * the context stream (pair_off[0] and pair_off[nrows] are read back first:
 * not monotone is SDNR_ERR_INVAL); on a multi-device context it runs on the
 * primary device.  nrows == 0 or no pairs: SDNR_OK, nothing touched.  A row
 * that is not a tree of the graph is reported by sdnr_synchronize as
 * SDNR_ERR_INVAL (the rounds are bounded; that row adds nothing). */
int sdnr_link_loads(sdnr_ctx *ctx, const void *tree, int32_t layout, int32_t nrows,
                    const int64_t *pair_off, const int32_t *dsts, const uint64_t *weight,
                    uint64_t *load, uint32_t flags);

/* Multicast trees: the one-to-many flow entries of groups and the loads they
 * put on the links.  OpenFlow 1.0 lets one flow entry carry several output
 * actions, so a switch can replicate; when a root sends to a group along the
 * controller's own routes, the links used are the SET UNION of the members'
 * routes -- the (dpid, out_port) entries Router._add_flows_for_path (reference
 * sdnmpi/router.py:83-104) would install for find_route(root, m) over the
 * members m, each once (the reference itself can only flood one-to-many
 * traffic, BroadcastRequest, sdnmpi/topology.py:150-177).  No route is built:
 * one lane per member walks its route through the table row and marks the
 * links in an E-bit map of the group (in LDS while V + E bits fit 32 KiB, else
 * in the context scratch); the union is that map.
 *   tree      [nrows][V] rows as sdnr_link_loads takes them: default-route
 *             trees in layout SDNR_TREE_INT32, SDNR_TREE_PORT16 or
 *             SDNR_TREE_SLOT; with SDNR_MCAST_TO_ROOT per-destination next-hop
 *             rows (nh of sdnr_shortest_tables / sdnr_cost_tables, layout
 *             SDNR_TREE_INT32 only);
 *   root      [ngroups] int32: the root switch of group g (dense id);
 *   mem_off   [ngroups + 1] int64: the members of group g are the pairs
 *             (mem_row[i], mem_vertex[i]), i in mem_off[g] .. mem_off[g+1);
 *             tree rows: mem_row[i] is the row of root[g]'s tree (the same for
 *             every member of the group), the route climbs parent() from
 *             mem_vertex[i] to the root and its links are parent(x) -> x;
 *             SDNR_MCAST_TO_ROOT: mem_row[i] is the row of destination
 *             mem_vertex[i], the route descends from root[g] along nh[mem_row[i]]
 *             and its links are x -> nh[x];
 *   weight    [ngroups] u64, NULL: all 1;
 *   reached   [mem_off[ngroups]] u8, may be NULL: 1 when member i's route
 *             exists -- tree rows: the member's own word is not SDNR_TREE_NONE
 *             (PORT16: its parent half is not 0xFFFF); SDNR_MCAST_TO_ROOT:
 *             nh[mem_row[i]][root[g]] >= 0 -- or when the member is the root
 *             (no link); 0 for an unreached member and for a root, row or
 *             vertex outside its range: these contribute nothing.  Repeated
 *             members count as one;
 *   ent_cnt   [ngroups] int64, may be NULL: the number of links of group g's
 *             union (0 for a group without members);
 *   ent_off, ent_edge  both NULL or both given: ent_off [ngroups + 1] int64 is
 *             the caller's exclusive prefix of ent_cnt, and the union of group
 *             g is written as int32 CSR edge ids, ascending, at ent_edge[
 *             ent_off[g] .. ent_off[g+1]) -- a count call, the prefix sum, then
 *             a fill call (the idiom of sdnr_route_offsets / sdnr_route_expand;
 *             the fill walks again, nothing is kept between the calls).  A group
 *             whose slice is not exactly its count, or leaves [ent_off[0],
 *             ent_off[ngroups]], is not written and sdnr_synchronize reports
 *             SDNR_ERR_INVAL;
 *   load      [E] u64 in the CSR's edge order, may be NULL: load[e] +=
 *             weight[g] once for every link e of group g's union.  The call
 *             ADDS into load (pass it to one of the two calls); sums wrap,
 *             bit-exact and order-independent.
 * Device pointers only (flags must hold SDNR_DEVICE_PTRS); asynchronous on
 * the context stream (the ends of mem_off and ent_off are read back first: not
 * monotone is SDNR_ERR_INVAL); on a multi-device context it runs on the
 * primary device.  ngroups == 0 or no members: SDNR_OK, nothing touched.
 * Every walk is bounded by V steps.  A walk that runs out (a parent cycle),
 * leaves [0, V), ends at a vertex that is not the root or steps over a pair
 * that is no link of the uploaded CSR marks a row that is not a tree of the
 * graph: sdnr_synchronize reports SDNR_ERR_INVAL, and the walk's whole group
 * contributes nothing (count 0, no edges, no load; the walks of a group share
 * their claims, so one walk's links cannot be taken back alone). */
#define SDNR_MCAST_TO_ROOT 0x40u /* sdnr_multicast_trees: rows are per-destination
                                  * next-hop rows, walked down from the root */
int sdnr_multicast_trees(sdnr_ctx *ctx, const void *tree, int32_t layout, int32_t nrows,
                         int32_t ngroups, const int32_t *root, const int64_t *mem_off,
                         const int32_t *mem_row, const int32_t *mem_vertex,
                         const uint64_t *weight, uint8_t *reached, int64_t *ent_cnt,
                         const int64_t *ent_off, int32_t *ent_edge, uint64_t *load,
                         uint32_t flags);

/* Per-link loads of a traffic matrix under ECMP: every pair's traffic is split
 * over ALL its shortest routes -- the set find_route(multiple=True) returns
 * (reference _find_routes_bfs, sdnmpi/util/topology_db.py:86-122) -- where
 * sdnr_link_loads puts it on one.  No route is enumerated and no count
 * saturates: per destination row the shortest-route counts sigma[] are a level
 * DP in double, and the demand is pushed down the shortest-path DAG level by
 * level, O(E) per row whatever the number of pairs or routes.
 *   dist      [nrows][V] u16 distance rows of sdnr_shortest_tables, row r = the
 *             hop counts toward one destination (SDNR_DIST_INF: unreached);
 *   pair_off  [nrows + 1] int64: the pairs of row r are srcs[pair_off[r] ..
 *             pair_off[r+1]) (source switches, dense ids) with weight[] (u64,
 *             e.g. bytes) at the same indices; weight NULL: all 1.  Weights
 *             are converted to double: values >= 2^53 round to nearest;
 *   load      [E] double in the uploaded CSR's edge order.  The call ADDS into
 *             load (the caller zeroes it; row chunks of one batch sum up).
 * A vertex x of level L = dist[x] > 0 has as next hops its out-neighbours of
 * level L - 1.  Default (route split): each of the pair's sigma[s] shortest
 * routes carries w / sigma[s], i.e. x sends the share sigma[n] / sigma[x] of
 * the flow through it over link x -> n.  SDNR_LOADS_SPLIT_HOP: x sends 1 /
 * (number of its next hops) over each (an OpenFlow select group per switch).
 * load[e(x -> n)] receives what is sent over it.  Unreachable sources, sources
 * outside [0, V), the pair s == d and zero weights contribute nothing;
 * repeated pairs add.  Sums are f64 atomics: every term is non-negative (the
 * relative error is a few ulp per level), but the last bits depend on the
 * order of arrival and may differ between runs unless every partial sum is
 * exact (power-of-two shares, integer weights).  No NaN or Inf reaches load.
 * Device pointers only (flags must hold SDNR_DEVICE_PTRS); asynchronous on
 * the context stream (pair_off[0] and pair_off[nrows] are read back first:
 * not monotone is SDNR_ERR_INVAL); on a multi-device context it runs on the
 * primary device.  nrows == 0 or no pairs: SDNR_OK, nothing touched.  A row
 * that is not a BFS labelling of the graph (a vertex of level > 0 without a
 * next hop, a level >= V, a route count above the double range) is reported
 * by sdnr_synchronize as SDNR_ERR_INVAL; that vertex's flow is dropped. */
int sdnr_ecmp_link_loads(sdnr_ctx *ctx, const uint16_t *dist, int32_t nrows,
                         const int64_t *pair_off, const int32_t *srcs, const uint64_t *weight,
                         double *load, uint32_t flags);

/* Per-link loads of a traffic matrix under ECMP over the LEAST-COST routes:
 * sdnr_ecmp_link_loads under the uploaded link costs (sdnr_graph_costs), what
 * an OSPF / IS-IS fabric with equal-cost multipath carries once links are
 * costed up or out -- where sdnr_link_loads over sdnr_cost_tables' nh rows puts
 * each pair on the one lexicographically smallest route.
 *   pcost     [nrows][V] u32 rows as sdnr_cost_tables writes them, row r = the
 *             least path costs toward one destination (SDNR_COST_INF: no route);
 *   pair_off, srcs, weight, load: as in sdnr_ecmp_link_loads.  The call ADDS
 *             into load.
 * Link e = (x -> n) is a next-hop link of x when pcost[n] != SDNR_COST_INF and
 * pcost[n] + cost[e] == pcost[x]; costs are >= 1, so these links form a DAG
 * toward the destination, but the next hops of a vertex need not sit one hop
 * count down (a direct link of cost 2 ties two links of cost 1): the vertices
 * are ordered by their longest next-hop chain: pull sweeps finalise the
 * vertices of chain length 1, 2, ... together with their route counts sigma[]
 * (double), and the demand is pushed down that order, O(E) per row for the
 * push and at most O(E) per sweep.  Default (route split): each of the
 * pair's sigma[s] least-cost routes carries w / sigma[s].
 * SDNR_LOADS_SPLIT_HOP: every switch sends 1 / (number of its next hops) over
 * each.  Unreachable sources, sources outside [0, V), the pair s == d and zero
 * weights contribute nothing; repeated pairs add.  Sums are f64 atomics: every
 * term is non-negative, but the last bits depend on the order of arrival and
 * may differ between runs unless every partial sum is exact (power-of-two
 * shares, integer weights).  No NaN or Inf reaches load.
 * Device pointers only (flags must hold SDNR_DEVICE_PTRS); asynchronous on
 * the context stream (pair_off[0] and pair_off[nrows] are read back first:
 * not monotone is SDNR_ERR_INVAL); on a multi-device context it runs on the
 * primary device; SDNR_TIMING as in sdnr_ecmp_link_loads.  Without an uploaded
 * graph or without uploaded costs: SDNR_ERR_STATE.  nrows == 0 or no pairs:
 * SDNR_OK, nothing touched.  One launch.  A row that is not a least-cost
 * labelling of the graph under the costs in force (a vertex of finite cost > 0
 * without a next hop, an ordering pass longer than V, a route count above the
 * double range) is reported by sdnr_synchronize as SDNR_ERR_INVAL; the
 * offending flow is dropped. */
int sdnr_cost_ecmp_link_loads(sdnr_ctx *ctx, const uint32_t *pcost, int32_t nrows,
                              const int64_t *pair_off, const int32_t *srcs,
                              const uint64_t *weight, double *load, uint32_t flags);

/* Link-failure what-if: sdnr_cost_ecmp_link_loads once per failure SCENARIO,
 * without touching the uploaded graph, its costs or any table.  A scenario is
 * a set of failed directed links; for every scenario k and destination row r
 * one workgroup computes the least costs toward dst[r] on the graph without
 * the scenario's links (pull Bellman-Ford, as sdnr_cost_tables), then orders
 * the least-cost DAG, counts the routes and pushes the row's demand down it
 * (as sdnr_cost_ecmp_link_loads), the failed links excluded at every step and
 * all of it in LDS: no table is written.
 *   dst        [nrows] the destination (dense id) of row r;
 *   pair_off, srcs, weight: as in sdnr_cost_ecmp_link_loads; with
 *              npairs = pair_off[nrows] - pair_off[0], pair i below is
 *              srcs[pair_off[0] + i];
 *   scen_off   [nscen + 1] int64: the failed links of scenario k are
 *              scen_edges[scen_off[k] .. scen_off[k+1]), CSR edge indices in
 *              [0, E), ascending within a scenario, duplicates allowed
 *              (scen_edges may be NULL when every scenario is empty);
 *   load       [nscen][E] double, slice k in the uploaded CSR's edge order.
 *              The call ADDS into load;
 *   lost       [nscen] double or NULL: the call ADDS the weight of every pair
 *              with a source in [0, V), s != d and weight > 0 that has no route
 *              in scenario k;
 *   routed     [nscen][npairs] u8 or NULL, WRITTEN for the pairs of every row
 *              that has pairs: 1 iff the source is in [0, V) and reaches the
 *              destination in scenario k (the pair s == d counts as routed).
 * Defining property: slice k equals sdnr_cost_ecmp_link_loads over
 * sdnr_cost_tables rows of the graph from which the links of scenario k were
 * really removed, scattered back to this graph's edge order; the links of the
 * scenario carry exactly 0.  That holds for a failed link that stays TIGHT too
 * (pcost[n] + cost == pcost[x] still holds for it when x keeps another next
 * hop of the same cost): it carries nothing and counts as no route.  The costs
 * are those of sdnr_graph_costs; with none uploaded every link costs 1 and the
 * routes are the hop-count ECMP routes.  An empty scenario is the fabric as it
 * is: sdnr_cost_ecmp_link_loads' result (sdnr_ecmp_link_loads' without costs).
 * Failures are directed: failing x -> n leaves n -> x up.
 * SDNR_LOADS_SPLIT_HOP, the sums (f64 atomics) and "no NaN or Inf reaches load
 * or lost" as in sdnr_cost_ecmp_link_loads.  Device pointers only (flags must
 * hold SDNR_DEVICE_PTRS); asynchronous on the context stream (the ends of
 * pair_off and scen_off are read back first: not monotone is SDNR_ERR_INVAL);
 * on a multi-device context it runs on the primary device; SDNR_TIMING as in
 * sdnr_ecmp_link_loads.  Without an uploaded graph: SDNR_ERR_STATE.  Negative
 * counts or NULL where a buffer is required: SDNR_ERR_INVAL.  nscen == 0,
 * nrows == 0 or no pairs: SDNR_OK, nothing touched.  A destination outside
 * [0, V) is an empty row: nothing added, its pairs not routed.  One launch.
 * A failed-link index outside [0, E) (that entry is ignored), a scenario that
 * is not ascending, offsets outside their lists, relaxation sweeps that outrun
 * V and a route count above the double range are reported by sdnr_synchronize
 * as SDNR_ERR_INVAL. */
int sdnr_failure_ecmp_link_loads(sdnr_ctx *ctx, const int32_t *dst, int32_t nrows,
                                 const int64_t *pair_off, const int32_t *srcs,
                                 const uint64_t *weight, int32_t nscen, const int64_t *scen_off,
                                 const int32_t *scen_edges, double *load, double *lost,
                                 uint8_t *routed, uint32_t flags);

/* Link-cost what-if: sdnr_cost_ecmp_link_loads once per COST scenario, without
 * touching the uploaded graph, its costs or any table, and optionally the peak
 * utilisation of every scenario.  A scenario is a set of cost overrides
 * (directed link, new cost); the new cost SDNR_COST_INF takes the link down,
 * so sdnr_failure_ecmp_link_loads is the special case of all-INF scenarios.
 * The work per (scenario, destination row) is sdnr_failure_ecmp_link_loads',
 * all of it in LDS, with the cost in force -- the base cost, the override, or
 * down -- read at every step: the Bellman-Ford, the ordering of the least-cost
 * DAG with its route counts, and the push.
 *   dst, nrows, pair_off, srcs, weight, load, lost, routed: as in
 *              sdnr_failure_ecmp_link_loads.  The call ADDS into load and lost;
 *   scen_off   [nscen + 1] int64: the overrides of scenario k are entries
 *              scen_off[k] .. scen_off[k+1] of scen_edges / scen_costs;
 *   scen_edges CSR edge indices in [0, E), STRICTLY ascending within a scenario;
 *   scen_costs parallel to scen_edges: the link's cost in this scenario, >= 1
 *              with cost * (V - 1) < SDNR_COST_INF (sdnr_graph_costs' rule), or
 *              SDNR_COST_INF: the link is down.  An override may lower a cost
 *              as well as raise it.  (Both lists may be NULL when every
 *              scenario is empty);
 *   capacity   [E] double or NULL (1.0 per link), read only for peak;
 *   peak       [nscen] double, WRITTEN: the max over e of load[k][e] /
 *              capacity[e], over load as it stands after this call's additions
 *              (0.0 when no link carries anything);
 *   peak_edge  [nscen] int32, WRITTEN: the smallest e that attains peak[k], -1
 *              when peak[k] is 0.  peak and peak_edge are both given or both
 *              NULL.
 * Defining property: slice k equals sdnr_cost_ecmp_link_loads over
 * sdnr_cost_tables rows of a graph with the costs of scenario k really
 * uploaded and its INF links really removed, scattered back to this graph's
 * edge order; a link that is down carries exactly 0, also one that stays tight
 * by its base cost.  The base cost of a link is the one sdnr_graph_costs
 * uploaded, 1 when none was.  An empty scenario, and an override equal to the
 * base cost, are the fabric as it is.  Overrides are directed.
 * SDNR_LOADS_SPLIT_HOP, the sums (f64 atomics) and "no NaN or Inf reaches load
 * or lost" as in sdnr_cost_ecmp_link_loads.  Device pointers only (flags must
 * hold SDNR_DEVICE_PTRS); asynchronous on the context stream (the ends of
 * pair_off and scen_off are read back first: not monotone is SDNR_ERR_INVAL);
 * on a multi-device context it runs on the primary device; SDNR_TIMING times
 * the main kernel (not the peak reduction), which sdnr_last_kernel names;
 * sdnr_last_launches is 1.  Without an uploaded graph: SDNR_ERR_STATE.
 * Negative counts, NULL where a buffer is required, one of peak / peak_edge
 * without the other: SDNR_ERR_INVAL.  nscen == 0: SDNR_OK, nothing touched.
 * nrows == 0 or no pairs: nothing is added; peak and peak_edge are still
 * written from load as it stands.  A destination outside [0, V) is an empty
 * row.  An override whose cost is 0 or breaks the cost rule, whose index is
 * outside [0, E) or is not greater than its predecessor's is IGNORED -- the
 * link keeps the cost it had -- and a capacity that is not finite or not > 0
 * has its link left out of the peak; either, and offsets outside their lists,
 * relaxation sweeps that outrun V or a route count above the double range, is
 * reported by sdnr_synchronize as SDNR_ERR_INVAL.  The other scenarios of the
 * call are unaffected and the context stays usable. */
int sdnr_whatif_ecmp_link_loads(sdnr_ctx *ctx, const int32_t *dst, int32_t nrows,
                                const int64_t *pair_off, const int32_t *srcs,
                                const uint64_t *weight, int32_t nscen, const int64_t *scen_off,
                                const int32_t *scen_edges, const uint32_t *scen_costs,
                                double *load, double *lost, uint8_t *routed,
                                const double *capacity, double *peak, int32_t *peak_edge,
                                uint32_t flags);

/* Loop-free alternate (fast-reroute) backup next hops per destination: the
 * neighbour a switch may hand a destination's traffic to the moment its
 * primary link dies, without the packet coming back (RFC 5286; an OpenFlow
 * fast-failover group's second bucket).  Integer and bit-exact.
 *   pcost_all  [V][V] u32, row v = sdnr_cost_tables' pcost row of destination
 *              v under the costs in force: P[d][x] = least cost x -> d,
 *              SDNR_COST_INF: no route.  With no costs uploaded every link
 *              costs 1 and the rows are hop counts;
 *   dst        [ndst] destinations (dense ids); row i of the outputs is dst[i];
 *   backup, backup_port [ndst][V] int32, kind [ndst][V] u8: WRITTEN;
 *   counts     [ndst][4] u32 or NULL: WRITTEN -- the row's primaries, backups,
 *              node-protecting backups and downstream backups.
 * The primary of (s, d) is p = the smallest out-neighbour of s with
 * cost(s -> p) + P[d][p] == P[d][s] (sdnr_cost_tables' nh); there is none at
 * s == d or where P[d][s] is SDNR_COST_INF.  A candidate is an out-link
 * e = (s -> n) with n != p and P[d][n] finite.  It is
 *   loop-free (link-protecting) iff P[s][n] is INF or P[d][n] < P[s][n] + P[d][s]
 *              (no least-cost route n -> d visits s),
 *   downstream iff P[d][n] < P[d][s],
 *   node-protecting iff loop-free and (P[p][n] is INF or
 *              P[d][n] < P[p][n] + P[d][p]) (no least-cost route n -> d visits
 *              p; never when p == d).
 * The backup is the loop-free candidate of the smallest key (not
 * node-protecting, cost[e] + P[d][n], n); with SDNR_LFA_LINK_ONLY the key is
 * (cost[e] + P[d][n], n).  backup = that n, backup_port = that link's port,
 * kind = 1 | downstream << 1 | node-protecting << 2; -1 / -1 / 0 where there is
 * no primary or no backup.  The sums are taken in 64 bits (two table entries
 * may reach 2^32) and INF enters none.
 * A pre-pass gathers P[s][n] per link and, unless SDNR_LFA_LINK_ONLY is set,
 * P[n_j][n_i] per pair of neighbours of a vertex (the sum of the squared
 * out-degrees, 4 bytes each) into the context scratch: more than 1 GiB of them
 * is SDNR_ERR_NOMEM (use SDNR_LFA_LINK_ONLY).  V is at most 16,384
 * (sdnr_apsp's cap: a 1 GiB table, a 64 KiB row in LDS), above it
 * SDNR_ERR_INVAL before anything is read: the fat-tree k=48 and the dragonfly
 * fit, the torus 32^3 and the 100k Jellyfish cannot hold an all-pairs table
 * and are out of scope.
 * Device pointers only (flags must hold SDNR_DEVICE_PTRS); asynchronous on the
 * context stream; on a multi-device context it runs on the primary device;
 * SDNR_TIMING times the main kernel (not the pre-pass).  Without an uploaded
 * graph: SDNR_ERR_STATE.  ndst == 0: SDNR_OK, nothing touched.  A dst[i]
 * outside [0, V) is an empty row (-1 / -1 / 0, counts 0).  A requested row
 * with P[d][d] != 0, or with a vertex of finite cost > 0 that has no tight
 * link (such a vertex gets no primary), is reported by sdnr_synchronize as
 * SDNR_ERR_INVAL; the other rows of the call are unaffected. */
int sdnr_lfa_tables(sdnr_ctx *ctx, const uint32_t *pcost_all, const int32_t *dst, int32_t ndst,
                    int32_t *backup, int32_t *backup_port, uint8_t *kind, uint32_t *counts,
                    uint32_t flags);

/* Remote loop-free alternates (RFC 7490): where no neighbour of a switch is
 * loop-free, the packet is tunnelled to a remote PQ node that is reached
 * without the failed link and reaches the link's far end without it.  One
 * repair per directed link.  Integer and bit-exact.
 *   pcost_all  [V][V] u32 as in sdnr_lfa_tables; D(a, b) = pcost_all[b][a] is
 *              the least cost a -> b, SDNR_COST_INF: no route.  With no costs
 *              uploaded every link costs 1;
 *   verts      [nverts] source vertices (dense ids), or NULL: 0 .. nverts - 1;
 *   pq, via, via_port [E] int32, tunnel_cost [E] u64, kind [E] u8, in CSR edge
 *              order: a unit (one source vertex S) WRITES the entries of S's
 *              out-links and touches no other; a vertex listed twice writes
 *              the same values twice;
 *   counts     [nverts][4] u32 or NULL: WRITTEN -- the unit's out-links that
 *              are no self-loops, those repaired, those with kind & 2, those
 *              with kind & 4.
 * For a link e = (S -> E) of cost c, E != S (a self-loop gets no repair):
 *   Q-space    X != S with D(X,E) finite and (D(X,S) INF or
 *              D(X,E) < D(X,S) + c): no least-cost route X -> E uses e;
 *   extended P-space through N, the head of an out-link f = (S -> N), N != E,
 *              N != S: D(N,X) finite and (D(N,S) INF or D(E,X) INF or
 *              D(N,X) < D(N,S) + c + D(E,X)): no least-cost route N -> X uses
 *              e (X = N qualifies).
 * The repair of e is the (X, N), X in the Q-space and in the extended P-space
 * through N, of the smallest key (cost[f] + D(N,X), X, N): pq = X, via = N,
 * via_port = f's port, tunnel_cost = cost[f] + D(N,X), kind = 1 | 2 where X is
 * in S's own P-space (D(S,X) finite and (D(E,X) INF or D(S,X) < c + D(E,X)):
 * the tunnel needs no directed forwarding) | 4 where X == N (a per-link
 * loop-free alternate, no tunnel); -1 / -1 / -1 / 0 / 0 where there is none.
 * Every sum is taken in 64 bits (three table entries may reach 3 (2^32 - 2))
 * and INF enters none.
 * A pre-pass transposes pcost_all into the context scratch (4 V^2 bytes; more
 * than 1 GiB is SDNR_ERR_NOMEM), so that the main kernel streams rows only.
 * V is at most 16,384 (sdnr_lfa_tables' cap), above it SDNR_ERR_INVAL before
 * anything is read.  Device pointers only (flags must hold SDNR_DEVICE_PTRS);
 * asynchronous on the context stream; on a multi-device context it runs on
 * the primary device; SDNR_TIMING times the main kernel (not the transpose).
 * Without an uploaded graph: SDNR_ERR_STATE.  nverts == 0: SDNR_OK, nothing
 * touched.  A verts[i] outside [0, V) is an empty unit (counts 0, no entry
 * written).  The table is taken as given: one that is no least-cost labelling
 * of the graph gives the repairs these inequalities define on it. */
int sdnr_remote_lfa(sdnr_ctx *ctx, const uint32_t *pcost_all, const int32_t *verts, int32_t nverts,
                    int32_t *pq, int32_t *via, int32_t *via_port, uint64_t *tunnel_cost,
                    uint8_t *kind, uint32_t *counts, uint32_t flags);

/* Fast-reroute what-if: the link loads of a demand while the switches' backup
 * next hops are forwarding -- after a failure, before the controller has
 * re-routed (sdnr_failure_ecmp_link_loads is the state after that).  Integer
 * and bit-exact.  Per (scenario k, destination row r), toward d = dst[r]:
 *   a switch x with nh[r][x] == -1 forwards nowhere, and so does d itself (its
 *   own two entries are not read);
 *   fwd(x) = nh[r][x] if the link x -> nh[r][x] is not in scenario k;
 *   else fwd(x) = backup[r][x] if that is not -1 and the link x -> backup[r][x]
 *   is not in the scenario either: a REPAIR;
 *   else x DROPS.
 * A pair (s, d) follows fwd from s.  Its status is
 *   0  no base route (following nh alone from s does not end at d), or s
 *      outside [0, V);
 *   1  delivered over primaries only (s == d included: it uses no link);
 *   2  delivered through at least one repair;
 *   3  dropped: the walk ends at a switch other than d;
 *   4  looped: the walk never ends.
 * Only DELIVERED pairs (status 1 or 2) add load: their weight on every link of
 * their walk.  A pair that is dropped or loops adds nothing to any link, as a
 * pair without a route adds nothing in sdnr_failure_ecmp_link_loads.
 *   dst        [nrows] the destination (dense id) of row r;
 *   nh, backup [nrows][V] int32: the rows sdnr_cost_tables (or
 *              sdnr_shortest_tables) and sdnr_lfa_tables write for dst, -1: none.
 *              They are taken as given: a backup need not be a loop-free
 *              alternate, and one that leads into a cycle gives status 4;
 *   pair_off, srcs, weight: as in sdnr_cost_ecmp_link_loads; pair i below is
 *              srcs[pair_off[0] + i], npairs = pair_off[nrows] - pair_off[0];
 *   nscen, scen_off, scen_edges: as in sdnr_failure_ecmp_link_loads -- CSR
 *              edge indices in [0, E), ascending within a scenario, duplicates
 *              allowed, directed;
 *   load       [nscen][E] u64.  The call ADDS (sums wrap: the order of the
 *              atomics does not matter);
 *   stat       [nscen][4] u64 or NULL.  The call ADDS the weight of the pairs
 *              of status 2 (repaired), 3 (dropped), 4 (looped) and 0 (no base
 *              route), in this order;
 *   status     [nscen][npairs] u8 or NULL, WRITTEN for the pairs of every row
 *              that has pairs;
 *   peak       [nscen] u64, WRITTEN: the largest load[k][e], over load as it
 *              stands after this call's additions;
 *   peak_edge  [nscen] int32, WRITTEN: the smallest e that attains peak[k], -1
 *              when peak[k] is 0.  Both are given or both are NULL.
 * Defining property: slice k equals sdnr_link_loads with SDNR_LOADS_TO_ROOT
 * over the rows fwd of scenario k and the delivered pairs.  An empty scenario
 * gives the loads of nh itself with every routed pair at status 1.
 * The loads of the rows without any failure are computed once per call and
 * added to every slice; then only the AFFECTED items are recomputed -- (k, r)
 * where row r has pairs and some link x -> n of scenario k has nh[r][x] == n --
 * one workgroup each with the row's state in LDS (26 bytes per vertex).
 * sdnr_last_frr_items reports their number.  There is no other form: V is at
 * most kFrrMaxV = 6,200 (the fat-tree k=48, the dragonfly a16 h8 p8 and the
 * 16^3 torus fit), above it SDNR_ERR_INVAL before anything is read.  The call
 * keeps one u64 per (row, vertex), 8 bytes per item and 12 per scenario entry
 * in the context scratch: more than 1 GiB is SDNR_ERR_NOMEM (split the
 * scenarios).
 * Device pointers only (flags must hold SDNR_DEVICE_PTRS); asynchronous on the
 * context stream (the ends of pair_off and scen_off are read back first: not
 * monotone is SDNR_ERR_INVAL); on a multi-device context it runs on the
 * primary device; SDNR_TIMING times the item kernel, which sdnr_last_kernel
 * names (not the base, the pre-pass or the peak reduction); sdnr_last_launches
 * is 1.  Without an uploaded graph: SDNR_ERR_STATE.  Negative counts, NULL
 * where a buffer is required, one of peak / peak_edge without the other:
 * SDNR_ERR_INVAL.  nscen == 0: SDNR_OK, nothing touched.  nrows == 0 or no
 * pairs: nothing is added; peak and peak_edge are still written from load as it
 * stands.  A destination outside [0, V) is an empty row: nothing added, its
 * pairs at status 0.
 * Reported by sdnr_synchronize as SDNR_ERR_INVAL, the other rows, scenarios
 * and items unaffected and the context usable:
 *   an nh row that is no in-tree of the graph (an entry >= V or equal to its
 *   own vertex, a cycle, a link the graph lacks under a vertex that carries
 *   demand) or whose pair_off lies outside the pair list: the row adds nothing
 *   to any slice or stat and its pairs read status 0;
 *   a backup in use that is < -1, >= V or no out-neighbour: that item adds
 *   nothing of its own -- the slice keeps the row's base loads and statuses;
 *   a failed-link index outside [0, E): that entry is ignored;
 *   a scenario that is not ascending or whose scen_off lies outside the list:
 *   it is taken as empty.
 * A forwarding loop that backup causes is data, not an error. */
int sdnr_frr_link_loads(sdnr_ctx *ctx, const int32_t *dst, const int32_t *nh,
                        const int32_t *backup, int32_t nrows, const int64_t *pair_off,
                        const int32_t *srcs, const uint64_t *weight, int32_t nscen,
                        const int64_t *scen_off, const int32_t *scen_edges, uint64_t *load,
                        uint64_t *stat, uint8_t *status, uint64_t *peak, int32_t *peak_edge,
                        uint32_t flags);

/* Least-loaded routes: per destination, inside the least-cost (ECMP) set, the
 * route whose busiest link is the least busy -- the controller's question
 * "given what the links carry now, which of the equal-cost routes should this
 * flow take".  Integer and bit-exact.
 *   pcost  [ndst][V] u32 rows as sdnr_cost_tables writes them under the costs
 *          in force (sdnr_graph_costs; none uploaded: every link costs 1 and
 *          the rows are hop counts), row i toward dst[i];
 *   util   [E] u32, the utilisation of every directed link in the uploaded
 *          CSR's edge order, in any unit, values in [0, 0xFFFFFFFE] (from host
 *          buffers a 0xFFFFFFFF is SDNR_ERR_INVAL; a device one reads as
 *          0xFFFFFFFE);
 *   bott, nh, nh_port [ndst][V]: WRITTEN.
 * Link e = (x -> n) is tight when pcost[n] != SDNR_COST_INF and pcost[n] +
 * cost[e] == pcost[x]: the links of the least-cost routes toward dst[i].
 *   bott[i*V+x]     min over tight e = (x -> n) of max(util[e], bott[n]); 0 at
 *                   dst[i], 0xFFFFFFFF where pcost[x] is SDNR_COST_INF: the
 *                   smallest achievable busiest-link utilisation over all
 *                   least-cost routes x -> dst[i];
 *   nh[i*V+x]       the n of the tight link with the smallest key
 *                   (max(util[e], bott[n]), util[e], n), compared
 *                   lexicographically -- the best bottleneck, then the emptier
 *                   first link, then the smaller neighbour (-1 for x == dst[i]
 *                   or unreachable);
 *   nh_port[i*V+x]  that link's port, links[x][nh].src.port_no.
 * Following nh from x gives a least-cost route whose busiest link carries
 * exactly bott[x].  A tight link lowers pcost strictly (costs are >= 1), so an
 * nh row is an in-tree toward dst[i] and sdnr_link_loads with
 * SDNR_LOADS_TO_ROOT takes it as it is.  With util all zero, or all equal, nh
 * and nh_port equal sdnr_cost_tables' bit for bit.  A link that is not tight
 * is never used, however empty it is.  nh and nh_port go together and may both
 * be NULL (bottlenecks only).
 * Host buffers: synchronous; SDNR_DEVICE_PTRS: asynchronous on the context's
 * stream; SDNR_TIMING as in sdnr_cost_tables.  Without an uploaded graph:
 * SDNR_ERR_STATE.  ndst == 0: SDNR_OK, nothing touched.  A destination outside
 * [0, V): SDNR_ERR_INVAL for host buffers (the ids are checked before anything
 * runs), an empty row (0xFFFFFFFF / -1 / -1, its pcost row not read) for
 * device ids.  One launch (pull sweeps over the tight links to the fixed
 * point: depth of the least-cost DAG + 1 of them); on a multi-device context
 * it runs on the primary device.  A requested row with pcost[dst[i]] != 0, or
 * with a vertex of finite cost > 0 that has no tight link, is reported by
 * sdnr_synchronize as SDNR_ERR_INVAL; the other rows of the call are
 * unaffected. */
int sdnr_widest_tables(sdnr_ctx *ctx, const uint32_t *pcost, const uint32_t *util,
                       const int32_t *dst, int32_t ndst, uint32_t *bott, int32_t *nh,
                       int32_t *nh_port, uint32_t flags);

/* Max-min fair rates of flows routed over single-path route tables: what each
 * pair gets when the flows share the links the way TCP or RoCE flows
 * approximately do, the link that limits it, and every link's carried rate.
 * A flow i is a pair of sdnr_link_loads -- row r of tree (same layouts, same
 * pair_off), vertex verts[i] -- with a multiplicity mult[i] (u64: that many
 * identical parallel flows; 0: absent; mult NULL: all 1; the caller keeps the
 * sum below 2^53) and up to two extra constraints extra[2*i], extra[2*i+1]:
 * indices in [E, E + nextra) into cap, -1 for none (extra NULL: none; e.g. the
 * two hosts' ports).  Its links are the tree links from verts[i] to the row's
 * root.  cap [E + nextra] holds positive finite doubles: the links' capacities
 * in the uploaded CSR's edge order, then the extras'.
 * Progressive filling, with rem = cap, used = 0, n_prev = 0, every flow alive;
 * round k = 0, 1, ...:
 *   1. n[e] = sum of mult over the alive flows that cross e (u64, exact);
 *   2. for k > 0: m = n_prev[e] - n[e], p = r_{k-1} * (double)m, used[e] += p,
 *      rem[e] = max(rem[e] - p, 0.0) -- the multiply, the add and the subtract
 *      each rounded on its own (no FMA);
 *   3. share[e] = rem[e] / n[e] where n[e] > 0, else +inf; r_k = min share;
 *      r_k == +inf ends the rounds;
 *   4. e is saturated iff share[e] == r_k; every alive flow that crosses a
 *      saturated link or extra gets rate r_k, round k and bott = the first
 *      saturated tree link walking from verts[i] toward the root, else
 *      extra[2*i] if saturated, else extra[2*i+1], and is dead; n_prev = n.
 * One more step 2 after the last round makes used final.  Every round kills a
 * flow, so there are at most min(flows, E + nextra) rounds.  The allocation is
 * the max-min fair one, which is unique; every step is deterministic, so the
 * results are bit-exact and repeatable (engine.fair_rates_host restates them).
 *   rate  [npairs] f64, bott [npairs] i32 (an index into cap), round [npairs]
 *         i32, at the flows' indices: WRITTEN for pair_off[0] .. pair_off[nrows];
 *   level [max_rounds] f64: level[k] = r_k, +inf from *nrounds on;
 *   used  [E + nextra] f64: the rate every link and extra carries;
 *   nrounds  HOST int32: the rounds run, written before the call returns.
 * A flow at the row's root (no link) without an extra: rate +inf, round -1,
 * bott -1.  A vertex outside [0, V) or unreached in its row, a multiplicity 0,
 * and every flow of a rejected row: rate 0.0, round -1, bott -1.  A vertex is
 * a root when it is its own parent; SDNR_LOADS_TO_ROOT rows (next-hop rows,
 * SDNR_TREE_INT32 only, the link is v -> nh[v]) hold -1 at the destination and
 * at unreachable vertices alike, so there a vertex without a next hop is taken
 * as the root: pass -1 as the vertex of a pair known to be unreachable.  If
 * max_rounds rounds do not finish the filling, the flows still alive keep rate
 * 0.0, bott -1 and round -2 and *nrounds is max_rounds.
 * Device pointers only (flags must hold SDNR_DEVICE_PTRS).  No grid-wide
 * barrier: a round is two launches on the context's stream (a row kernel in
 * sdnr_link_loads' shape -- sdnr_last_kernel names its form,
 * "fair_rows_kernel<lds>" or "fair_rows_kernel<global>" -- and a kernel over
 * the E + nextra entries); rounds are queued in batches and the call waits for
 * an 8-byte status word per batch, so it returns when the rounds are done
 * (rate, bott, round and used are final then; level after sdnr_synchronize).
 * sdnr_last_launches gives the launches of the call.  On a multi-device
 * context it runs on the primary device.  nrows == 0 or no pairs: SDNR_OK,
 * *nrounds = 0, nothing else touched.  pair_off[0] > pair_off[nrows] is
 * SDNR_ERR_INVAL at once.  A row that is not a tree of the graph (every vertex
 * with a parent must have that link), offsets of a row outside the pair list,
 * a capacity that is not positive and finite (taken as +inf) and an extra
 * outside [E, E + nextra) (ignored) are reported by sdnr_synchronize as
 * SDNR_ERR_INVAL; the doublings are bounded and such a row adds nothing. */
int sdnr_fair_rates(sdnr_ctx *ctx, const void *tree, int32_t layout, int32_t nrows,
                    const int64_t *pair_off, const int32_t *verts, const uint64_t *mult,
                    const int32_t *extra /* [npairs][2] or NULL */, const double *cap,
                    int32_t nextra, double *rate, int32_t *bott, int32_t *round,
                    double *level, int32_t max_rounds, double *used,
                    int32_t *nrounds /* host */, uint32_t flags);

/* Max-min fair completion times: when every flow of an exchange ends.  The
 * fluid model behind sdnr_fair_rates has an exact answer: the flows share
 * max-min fairly, a flow that has sent its bytes leaves, the others are
 * refilled.  This is the one statement of the definition; fair_times.hip and
 * engine.fair_times_host follow it step for step.
 * Flows and initial classification.  Flows, multiplicities, extras,
 * capacities, rows, layouts and SDNR_LOADS_TO_ROOT are exactly those of
 * sdnr_fair_rates.  Each flow also has bytes[i], an f64 that is finite and
 * >= 0: the size of each of the flow's mult[i] identical parallel flows.
 * rem_b[i] = bytes[i], t = 0.0, carried[e] = 0.0 over the E + nextra entries.
 *   - Absent flows, with time = +inf, epoch = -1, rate0 = 0.0: a vertex
 *     outside [0, V) or unreached in its row; multiplicity 0; every flow of a
 *     rejected row.
 *   - A routed flow at its row's root with no extra: time = 0.0, epoch = -1,
 *     rate0 = +inf.
 *   - A routed flow with bytes == 0: time = 0.0, epoch = -1.  It never takes
 *     part in the sharing.  Its rate0 is what sdnr_fair_rates gives the same
 *     call with that flow's multiplicity set to 0 (0.0).
 *   - Every other flow is in flight.
 * Epoch j = 0, 1, ...:
 *   1. Fill.  sdnr_fair_rates' progressive filling, steps 1-4 and the closing
 *      step 2, unchanged and with the same operation order, over the flows in
 *      flight: rate[i], the epoch's used[e] and its round count.  rate0 is the
 *      rate of epoch 0 (with max_epochs == 0 no filling runs and the flows in
 *      flight keep rate0 = 0.0).
 *   2. Advance.  q[i] = rem_b[i] / rate[i]; dt = min q over the flows in
 *      flight; t_j = t_{j-1} + dt; carried[e] += used[e] * dt, the multiply and
 *      the add each rounded on their own (no FMA).  A flow finishes iff
 *      q[i] == dt, or rem_b[i] - rate[i] * dt <= 0.0 with the multiply and the
 *      subtract rounded separately: it gets time = t_j, epoch = j and leaves.
 *      Otherwise rem_b[i] becomes that difference.
 *   3. End when nothing is in flight.  Every epoch removes a flow, so there are
 *      at most as many epochs as flows.
 * The epoch cap.  When max_epochs epochs have run and flows are still in
 * flight, those keep time = +inf and epoch = -2, their remaining[i] is what is
 * left, and *nepochs = max_epochs.
 * Ties.  There is no tie tolerance, as in sdnr_fair_rates: flows that end at
 * the same instant as fractions may round one ulp of dt apart and then leave
 * in two consecutive epochs.  Each such epoch costs a filling and changes no
 * time beyond rounding.
 *   time [npairs] f64, epoch [npairs] i32, rate0 [npairs] f64, remaining
 *         [npairs] f64 (0.0 for a flow that finished, bytes[i] for an absent
 *         one), at the flows' indices: WRITTEN for pair_off[0] ..
 *         pair_off[nrows];
 *   epoch_time [max_epochs] f64, epoch_rounds [max_epochs] i32: t_j and the
 *         rounds of epoch j's filling, written for j < *nepochs;
 *   carried [E + nextra] f64: the bytes every link and extra carried;
 *   nepochs  HOST int32: the epochs run, written before the call returns.
 * Device pointers only (flags must hold SDNR_DEVICE_PTRS), on the primary
 * device of a multi-device context.  No grid-wide barrier, and the host knows
 * neither the round nor the epoch: a clock in device memory (phase, epoch,
 * round) tells every queued launch what to do, and the last workgroup of an
 * entry pass advances it.  A step is two launches on the context's stream (a
 * row kernel -- sdnr_last_kernel names its form, "fair_times_rows_kernel<lds>"
 * or "fair_times_rows_kernel<global>", chosen as in sdnr_fair_rates -- and a
 * kernel over the E + nextra entries).  Epoch j with K_j = epoch_rounds[j]
 * rounds takes K_j + 2 steps and the step that finds nothing in flight (or the
 * cap reached) one more: S = sum over j < *nepochs of (K_j + 2), plus 1.  Steps
 * are queued 16 at a time and the call waits for the clock's 16 bytes per
 * batch, so it returns when the epochs are done (every output is final then)
 * and sdnr_last_launches is 1 + 32 * ceil(S / 16).  SDNR_TIMING as in
 * sdnr_fair_rates.  nrows == 0 or no pairs: SDNR_OK, *nepochs = 0, nothing
 * else touched.  pair_off[0] > pair_off[nrows] is SDNR_ERR_INVAL at once.  A
 * row that is not a tree of the graph, offsets of a row outside the pair list,
 * a capacity that is not positive and finite (taken as +inf), an extra outside
 * [E, E + nextra) (ignored) and a byte size that is negative or not finite
 * (that flow is absent) are reported by sdnr_synchronize as SDNR_ERR_INVAL;
 * the other rows' flows are what they are without such a row. */
int sdnr_fair_times(sdnr_ctx *ctx, const void *tree, int32_t layout, int32_t nrows,
                    const int64_t *pair_off, const int32_t *verts, const uint64_t *mult,
                    const double *bytes, const int32_t *extra /* [npairs][2] or NULL */,
                    const double *cap, int32_t nextra, double *time, int32_t *epoch,
                    double *rate0, double *remaining, double *epoch_time /* [max_epochs] */,
                    int32_t *epoch_rounds /* [max_epochs] */, int32_t max_epochs,
                    double *carried /* [E + nextra] */, int32_t *nepochs /* host */,
                    uint32_t flags);

/* Max-min fair rates of flows split over EVERY least-cost route (ECMP): what
 * sdnr_fair_rates answers for one path per pair, for the fabric as it is run.
 * This is the one statement of the definition; ecmp_fair_rates.hip and
 * engine.ecmp_fair_rates_host follow it step for step.
 * Flows and fractions.  A flow i is a pair of sdnr_cost_ecmp_link_loads -- row
 * r of pcost (u32 least-cost rows toward one destination, SDNR_COST_INF: no
 * route; same pair_off), source vertex srcs[i] -- with sdnr_fair_rates'
 * multiplicity mult[i] (u64; 0: absent; NULL: all 1; the sum below 2^53) and up
 * to two extras extra[2*i], extra[2*i+1]: indices in [E, E + nextra) into cap,
 * -1 for none (extra NULL: none).  Link e = (x -> n) is TIGHT in the row when
 * pcost[n] != INF and pcost[n] + cost[e] == pcost[x].  The flow's links are the
 * tight links reachable from its source over tight links, and its fraction
 * phi_i(e) on each is what sdnr_cost_ecmp_link_loads would put there for unit
 * weight: route split (sigma[n] / sigma[x] down the DAG, sigma = the number of
 * least-cost routes to the destination) or, with SDNR_LOADS_SPLIT_HOP, hop
 * split (evenly over the next hops of every vertex).  The costs are those of
 * sdnr_graph_costs; with none uploaded every link costs 1, as
 * sdnr_failure_ecmp_link_loads takes it, so hop-count ECMP is the same call over
 * distance rows widened to u32.  Every tight link out of a vertex that holds
 * flow carries a positive fraction under both splits, so "flow i crosses e" is
 * combinatorial: e is tight and its tail is reachable from the source over
 * tight links.  cap [E + nextra]: positive finite doubles, the links' in the
 * uploaded CSR's edge order, then the extras'.
 * Filling.  rem = cap, used = 0, a_prev = 0, r_{-1} = 0, every flow alive;
 * round k = 0, 1, ...:
 *   1. a[e] = sum over the alive flows of mult * phi(e), in f64: the ECMP push
 *      of the alive multiplicities; for an extra the alive multiplicity itself;
 *   2. for k > 0: m = max(a_prev[e] - a[e], 0), p = r_{k-1} * m, used[e] += p,
 *      rem[e] = max(rem[e] - p, 0) -- every operation rounded on its own (no
 *      FMA);
 *   3. share[e] = rem[e] / a[e] where a[e] > 0, else +inf;
 *      r_k = max(min share, r_{k-1}); r_k == +inf ends the rounds;
 *   4. e is saturated iff share[e] <= r_k + r_k * kFairTie, kFairTie = 2^-30
 *      (the multiply and the add rounded one by one);
 *   5. every alive flow that crosses a saturated link or has a saturated extra
 *      gets rate r_k, round k and bott = the smallest saturated link index it
 *      crosses, else extra[2*i] if saturated, else extra[2*i+1], and is dead;
 *      a_prev = a.
 * One more step 2 after the last round makes used final.  The link with the
 * smallest share is saturated and some alive flow crosses it, so every round
 * kills a flow: at most min(flows, E + nextra) rounds.
 * Why a tolerance.  a[e] is a float sum, so two links whose shares are equal as
 * fractions differ in their last bits; under ECMP on a symmetric fabric that is
 * every link of a tier, and sdnr_fair_rates' exact share == r_k would saturate
 * each in a round of its own.  2^-30 is about 1e-9, the relative tolerance of
 * the ECMP loads, five orders above their measured summation error: what is not
 * flagged keeps a margin far above the noise in rem.  The clamp of step 3 makes
 * the levels non-decreasing by construction.  The consequence: a flow whose
 * own level lies within 2^-30 (relative) of r_k is frozen at r_k.
 * Reproducibility.  The adds into a[e] arrive in any order: results equal the
 * restatement within rounding, and bit for bit where every partial sum is exact
 * (power-of-two shares and integer multiplicities).
 *   rate, bott, round, level, used, nrounds, max_rounds: as in sdnr_fair_rates.
 * A flow with srcs[i] the destination (pcost 0) and no extra: rate +inf, round
 * -1, bott -1.  A source outside [0, V) or without a route, a multiplicity 0,
 * and every flow of a rejected row: rate 0.0, round -1, bott -1.  If max_rounds
 * rounds do not finish the filling, the flows still alive keep rate 0.0, bott
 * -1 and round -2 and *nrounds is max_rounds.
 * Device pointers only (flags must hold SDNR_DEVICE_PTRS).  No grid-wide
 * barrier: a round is two launches on the context's stream (a row kernel in
 * sdnr_cost_ecmp_link_loads' shape -- sdnr_last_kernel names its form,
 * "ecmp_fair_rows_kernel<lds>" or "ecmp_fair_rows_kernel<global>" -- and a
 * kernel over the E + nextra entries); batching behind an 8-byte status word,
 * sdnr_last_launches, SDNR_TIMING and the multi-device rule as in
 * sdnr_fair_rates.  nrows == 0 or no pairs: SDNR_OK, *nrounds = 0, nothing else
 * touched.  pair_off[0] > pair_off[nrows] is SDNR_ERR_INVAL at once.  A row that
 * is not a least-cost labelling of the graph under the costs in force (a vertex
 * of finite cost > 0 without a next hop, an ordering pass longer than V, a route
 * count above the double range: its flows read 0.0 / -1 / -1 and it adds
 * nothing), offsets of a row outside the pair list, a capacity that is not
 * positive and finite (taken as +inf) and an extra outside [E, E + nextra)
 * (ignored) are reported by sdnr_synchronize as SDNR_ERR_INVAL. */
int sdnr_ecmp_fair_rates(sdnr_ctx *ctx, const uint32_t *pcost, int32_t nrows,
                         const int64_t *pair_off, const int32_t *srcs, const uint64_t *mult,
                         const int32_t *extra /* [npairs][2] or NULL */, const double *cap,
                         int32_t nextra, double *rate, int32_t *bott, int32_t *round,
                         double *level, int32_t max_rounds, double *used,
                         int32_t *nrounds /* host */, uint32_t flags);

/* Max-min fair completion times over ECMP: when every flow of an exchange ends
 * if each is split over EVERY least-cost route -- what sdnr_fair_times answers
 * for one path per pair, for the fabric as it is run.  This is the one
 * statement of the definition; ecmp_fair_times.hip and
 * engine.ecmp_fair_times_host follow it step for step.
 * Flows and initial classification.  Flows, fractions, multiplicities, extras,
 * capacities, costs (none uploaded: every link costs 1) and
 * SDNR_LOADS_SPLIT_HOP are exactly those of sdnr_ecmp_fair_rates.  Each flow
 * also has bytes[i], as in sdnr_fair_times: an f64 that is finite and >= 0, the
 * size of each of the flow's mult[i] identical parallel flows.  rem_b[i] =
 * bytes[i], t = 0.0, carried[e] = 0.0 over the E + nextra entries.
 *   - Absent flows, with time = +inf, epoch = -1, rate0 = 0.0: a source outside
 *     [0, V) or without a route; multiplicity 0; a byte size that is negative or
 *     not finite; every flow of a row that is no least-cost labelling.
 *   - A routed flow at the destination (pcost 0) with no extra: time = 0.0,
 *     epoch = -1, rate0 = +inf, remaining = 0.0.
 *   - A routed flow with bytes == 0: time = 0.0, epoch = -1.  It never takes
 *     part in the sharing.  It is classified with its own multiplicity first,
 *     so at the destination without an extra it reads as the flow above
 *     (rate0 = +inf); anywhere else its rate0 is 0.0, the preset, since no
 *     filling ever counts it.
 *   - Every other flow is in flight.
 * Epoch j = 0, 1, ...:
 *   1. Fill.  sdnr_ecmp_fair_rates' filling over the flows in flight, steps 1-5
 *      and the closing step 2, unchanged and in the same operation order,
 *      kFairTie included: rate[i], the epoch's used[e] and its round count.
 *      rate0 is the rate of epoch 0 (with max_epochs == 0 no filling runs and
 *      the flows in flight keep rate0 = 0.0).
 *   2. Advance.  q[i] = rem_b[i] / rate[i]; dt = min q over the flows in
 *      flight; bound = dt + dt * kFairTie, the multiply and the add rounded one
 *      by one (step 4's rule); t_j = t_{j-1} + dt; carried[e] += used[e] * dt,
 *      the multiply and the add each rounded on their own (no FMA).  A flow
 *      finishes iff q[i] <= bound, or rem_b[i] - rate[i] * dt <= 0.0 with the
 *      multiply and the subtract rounded separately: it gets time = t_j, epoch
 *      = j, remaining = 0 and leaves.  Otherwise rem_b[i] becomes that
 *      difference.
 *   3. End when nothing is in flight.  Every epoch removes a flow, so there are
 *      at most as many epochs as flows.
 * The epoch cap, max_epochs, epoch = -2, remaining, nepochs, epoch_time and
 * epoch_rounds are as in sdnr_fair_times.
 * Why the advance shares the tolerance.  Under ECMP a[e] is a float sum whose
 * adds arrive in any order, so the levels of the device and of the restatement
 * differ in their last bits, and with them the q of flows that end together as
 * fractions.  With sdnr_fair_times' exact q == dt every such pair of flows would
 * leave in one epoch on one side and in two on the other, and each spurious
 * epoch costs a full refill with its DAG sweeps.  With the tolerance the
 * membership of an epoch flips only at q ~ dt * (1 + 2^-30), not at every exact
 * tie: the statement sdnr_ecmp_fair_rates makes for its levels.  The
 * consequence for carried: a flow that leaves within the tolerance has sent at
 * least rem_b / (1 + 2^-30), so carried[e] may fall short of the sum of mult *
 * bytes * phi(e) over the finished flows by at most 2^-30 relative, and exceeds
 * it only by rounding.
 *   time, epoch, rate0, remaining [npairs], epoch_time, epoch_rounds
 *   [max_epochs], carried [E + nextra], nepochs (HOST): as in sdnr_fair_times.
 *   There is no bottleneck output.
 * Device pointers only (flags must hold SDNR_DEVICE_PTRS), on the primary
 * device of a multi-device context.  No grid-wide barrier: sdnr_fair_times'
 * clock in device memory (phase, epoch, round) tells every queued launch what
 * to do, and the last workgroup of an entry pass advances it.  A step is two
 * launches on the context's stream (a row kernel in sdnr_ecmp_fair_rates' shape
 * -- sdnr_last_kernel names its form, "ecmp_fair_times_rows_kernel<lds>" or
 * "ecmp_fair_times_rows_kernel<global>" -- and a kernel over the E + nextra
 * entries); the steps of an epoch, the batches of 16 behind the clock's 16
 * bytes and sdnr_last_launches = 1 + 32 * ceil(S / 16) are those of
 * sdnr_fair_times.  SDNR_TIMING as there.  nrows == 0 or no pairs: SDNR_OK,
 * *nepochs = 0, nothing else touched.  pair_off[0] > pair_off[nrows] is
 * SDNR_ERR_INVAL at once.  A row that is not a least-cost labelling of the
 * graph under the costs in force (its flows are absent), offsets of a row
 * outside the pair list, a capacity that is not positive and finite (taken as
 * +inf), an extra outside [E, E + nextra) (ignored) and a byte size that is
 * negative or not finite (that flow is absent) are reported by
 * sdnr_synchronize as SDNR_ERR_INVAL; the other rows' flows are what they are
 * without such a row. */
int sdnr_ecmp_fair_times(sdnr_ctx *ctx, const uint32_t *pcost, int32_t nrows,
                         const int64_t *pair_off, const int32_t *srcs, const uint64_t *mult,
                         const double *bytes, const int32_t *extra /* [npairs][2] or NULL */,
                         const double *cap, int32_t nextra, double *time, int32_t *epoch,
                         double *rate0, double *remaining,
                         double *epoch_time /* [max_epochs] */,
                         int32_t *epoch_rounds /* [max_epochs] */, int32_t max_epochs,
                         double *carried /* [E + nextra] */, int32_t *nepochs /* host */,
                         uint32_t flags);

/* Flood ports (TopologyManager._is_edge_port / _do_broadcast, reference
 * sdnmpi/topology.py:150-177): is_edge[i] = 1 iff ports[i] is neither end of
 * any link.  Keys are (dense switch id << 32) | port_no; ends (both ends of
 * every link, the reference's link.src and link.dst) must be sorted
 * ascending (duplicates allowed).  Needs no uploaded graph. */
int sdnr_edge_ports(sdnr_ctx *ctx, const uint64_t *ends, int32_t nends,
                    const uint64_t *ports, int32_t nports, uint8_t *is_edge,
                    uint32_t flags);

/* Device time in milliseconds of the main kernel(s) of the last table call
 * made with SDNR_TIMING (waits for that call to finish). */
int sdnr_last_kernel_ms(sdnr_ctx *ctx, float *ms);

/* Number of launches of the main kernel in the last table call: the
 * min-plus squaring passes of sdnr_apsp, the BFS levels of the level-by-level
 * shortest kernel, 1 for single-launch kernels (0 before the first call). */
int sdnr_last_launches(const sdnr_ctx *ctx, int32_t *launches);

/* Number of workgroups in the last launch of a row-persistent kernel: the
 * kernels of sdnr_link_loads, sdnr_ecmp_link_loads, sdnr_cost_ecmp_link_loads,
 * sdnr_cost_tables, sdnr_widest_tables, sdnr_failure_ecmp_link_loads,
 * sdnr_whatif_ecmp_link_loads, sdnr_lfa_tables, sdnr_fair_rates,
 * sdnr_ecmp_fair_rates, sdnr_fair_times, sdnr_ecmp_fair_times (their row
 * kernel), sdnr_multicast_trees, sdnr_remote_lfa (its units are source vertices),
 * sdnr_frr_link_loads (its item kernel, over the affected items) and
 * sdnr_ecmp_counts give every workgroup the rows (batches, items, groups) r,
 * r + grid, r + 2 * grid, ...: with more units of work than this a workgroup
 * takes more than one.  The other entry points leave it as it was (0 before
 * the first such call). */
int sdnr_last_grid(const sdnr_ctx *ctx, int64_t *workgroups);

/* Sources the last sdnr_dfs_tables* call searched (waits for that call): the
 * batch size, or, when the call folded twin classes, one per class present
 * in the batch -- the other rows were derived (0 before the first call). */
int sdnr_last_dfs_searched(sdnr_ctx *ctx, int32_t *n);

/* (Scenario, row) items the last sdnr_frr_link_loads call recomputed (waits
 * for that call): the affected items, each once; 0 when the call had nothing
 * to do, and before the first call. */
int sdnr_last_frr_items(sdnr_ctx *ctx, int64_t *items);

/* Form of the search kernel in the last sdnr_dfs_tables* call: 0 the
 * full-load form, 1 the low-load form -- a folded call whose previous call on
 * this context (same graph upload, same batch size) left few live searches
 * (does not wait; both forms compute the same tables). */
int sdnr_last_dfs_form(const sdnr_ctx *ctx, int32_t *form);

/* Whether the search kernel of the last sdnr_dfs_tables* call ran on the
 * graph's twin-class quotient (1) or on the graph itself (0): the quotient is
 * taken where the graph has twins and its quotient at most half the links
 * (SDNROUTE_DFS_QUOTIENT=0|1 forces it; does not wait; the tables are the
 * same either way). */
int sdnr_last_dfs_quotient(const sdnr_ctx *ctx, int32_t *on);

/* Bellman-Ford sweeps of the last sdnr_apsp call (the most any 8-row block
 * ran, summed over its relaxation launches; 0 with SDNROUTE_APSP_RELAX=0). */
int sdnr_last_sweeps(const sdnr_ctx *ctx, int32_t *sweeps);

/* Name of the kernel variant the last table call launched on this context
 * (e.g. "dfs_count_kernel<4>"; "" before the first call). */
const char *sdnr_last_kernel(const sdnr_ctx *ctx);

#ifdef __cplusplus
}
#endif

#endif /* SDNROUTE_H */
