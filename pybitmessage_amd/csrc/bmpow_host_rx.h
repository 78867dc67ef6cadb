// bmpow_host_rx.h -- the msg family of the rows pipeline (bmpow_host_rows.h), internal.  Used by
// bmpow_host_rx.hip (bmpow_rx_msgs, which uploads the plaintexts: run_rows<RxFamily>) and
// bmpow_host_rxopen.hip (bmpow_rx_sealed_msgs, whose opening kernel leaves them on the device: grow_set,
// launch_set and phase_times over RxBufs).
#pragma once
#include "bmpow_host_rows.h"

#include "../../include/bmpow_rx.h"
#include "bmpow_rx_kernels.h"

namespace bmhost {

struct RxFamily {
  using Row = rx_row;
  using Pk = rx_pk;
  using Rec = bmpow_rx_msg_rec;
  static constexpr auto walk = rx_launch_walk;
  static constexpr auto pack = rx_launch_pack;
  static constexpr auto finish = rx_launch_finish;
};
using RxBufs = RowBufs<RxFamily>;

}  // namespace bmhost
