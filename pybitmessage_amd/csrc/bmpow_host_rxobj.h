// bmpow_host_rxobj.h -- the broadcast and pubkey family of the rows pipeline (bmpow_host_rows.h), internal.  Used
// by bmpow_host_rxobj.hip (bmpow_rx_objects, which uploads the plaintexts: run_rows<RxoFamily>) and
// bmpow_host_rxobjopen.hip (bmpow_rx_sealed_objects, whose opening kernel leaves them on the device: grow_set,
// launch_set and phase_times over RxoBufs; its clear pubkeys go through run_rows as well).
#pragma once
#include "bmpow_host_rows.h"

#include "../../include/bmpow_rx.h"
#include "bmpow_rx_fmt.h"
#include "bmpow_rxobj_kernels.h"

namespace bmhost {

struct RxoFamily {
  using Row = rxo_row;
  using Pk = rxo_pk;
  using Rec = bmpow_rx_obj_rec;
  static constexpr auto walk = rxo_launch_walk;
  static constexpr auto pack = rxo_launch_pack;
  static constexpr auto finish = rxo_launch_finish;
};
using RxoBufs = RowBufs<RxoFamily>;

}  // namespace bmhost
