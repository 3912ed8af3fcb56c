"""Operator tasks and the plugin API they register through.

Reference (OPS = src/handlers/operator_handler/operators):
  TaskBuilder trait                         OPS/traits.rs:22-36
  OperatorTaskRegistry                      OPS/operator_task_registry.rs:40-162
  FilterConfig / FilterTask / FilterTaskBuilder        OPS/filter_tasks/{config.rs, filter_task.rs:30-199}
  MaterializeFilesConfig / MaterializeFilesTask / ...  OPS/materialize_tasks/{config.rs, materialize_files_task.rs:30-230}
  OperatorTask::{Filter{expr}, MaterializeFiles{data_format, fields}}  src/planner/physical_planner.rs:58-65
  BlockingTask                              not in the reference: the protocol of the four operators below, which need every
                                            input row before they can send one (hold all / compute once / send / ack all)
  OrderByOperatorTask / OrderByTask         not in the reference (its DEV_NOTES.md lists ORDER BY as the next operator):
                                            `record_utils.sort_records`
  AggregateOperatorTask / AggregateTask     not in the reference either: GROUP BY, `record_utils.aggregate_records`
  WindowOperatorTask / WindowTask           not in the reference either: window functions (fn(...) OVER (...)),
                                            `record_utils.window_records` + `project_record`
  JoinOperatorTask / JoinTask               not in the reference either: JOIN (inner, left, right, full, semi, anti) of two
                                            inbound exchanges, `record_utils.join_records`

The hot loops call `record_utils.filter_record` / `project_record` exactly where the reference does
(filter_task.rs:99, materialize_files_task.rs:110); here those are the HIP kernels.  The control plane around
them (message router, pipes, TCP) is out of scope: `build` receives the exchanges directly.

What every task shares is written once: `_task_of` and `_max_rows_per_record` (the checks of the `try_from` methods),
`_LazyContext` (the library context, made on first use), `_runner` (what `TaskBuilder.build` returns) and, for the blocking
operators, `BlockingTask.async_main` -- the one place that says "ack only after every send, so a failure requeues the inputs".
"""
from __future__ import annotations

import abc
import dataclasses
import os
import uuid
from typing import Any, Callable, List, Optional, Sequence

from .. import record_utils
from .. import sqlast as A
from .exchange_operator import ExchangeOperator
from .record_handler import RecordHandler


# ---- planner types the tasks consume ------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class FilterOperatorTask:
    """planner::OperatorTask::Filter { expr }"""
    expr: A.Expr

    def task_name(self) -> str:
        return "filter"


@dataclasses.dataclass(frozen=True)
class MaterializeFilesOperatorTask:
    """planner::OperatorTask::MaterializeFiles { data_format, fields }"""
    data_format: str
    fields: Sequence[A.SelectItem]

    def task_name(self) -> str:
        return "materialize_files"


@dataclasses.dataclass(frozen=True)
class ReadFilesOperatorTask:
    """planner::OperatorTask::TableFunc { alias, func_name: "read_files", args, max_rows_per_batch } with the path argument
    already parsed (ReadFilesConfig::parse_config, read_files_task.rs:66-107)"""
    path: str                       # glob below the connection's root
    alias: Optional[str] = None
    max_rows_per_batch: int = 10_000   # physical_planner.rs:323

    def task_name(self) -> str:
        return "read_files"


@dataclasses.dataclass(frozen=True)
class OrderByOperatorTask:
    """ORDER BY keys [LIMIT n] (the reference's planner has no such task yet; shaped like its siblings)"""
    order_by: Sequence[A.OrderByExpr]
    limit: Optional[int] = None
    max_rows_per_record: int = 10_000   # physical_planner.rs:323 (the records the read_files task sends)

    def task_name(self) -> str:
        return "order_by"


@dataclasses.dataclass(frozen=True)
class AggregateOperatorTask:
    """GROUP BY keys with the output items of the SELECT list (`sqlparse.aggregate_plan`); shaped like OrderByOperatorTask.
    With HAVING (`sqlparse.having_plan`): `having` is the predicate over the output columns of `items`, of which the first
    `n_visible` are the SELECT list's (None: all of them)."""
    keys: Sequence[A.Expr]
    items: Sequence[A.AggItem]
    max_rows_per_record: int = 10_000
    having: Optional[A.Expr] = None
    n_visible: Optional[int] = None

    def task_name(self) -> str:
        return "aggregate"


@dataclasses.dataclass(frozen=True)
class WindowOperatorTask:
    """One window specification with the items and the final projection of the SELECT list (`sqlparse.window_plan`); shaped
    like AggregateOperatorTask"""
    partition_by: Sequence[A.Expr]
    order_by: Sequence[A.OrderByExpr]
    items: Sequence[A.WindowItem]
    projection: Sequence[A.SelectItem]
    max_rows_per_record: int = 10_000

    def task_name(self) -> str:
        return "window"


@dataclasses.dataclass(frozen=True)
class JoinOperatorTask:
    """JOIN on the (left column, right column) pairs of the ON condition (`sqlparse.join_plan`); inbound exchange 0
    is the left input, 1 the right; shaped like AggregateOperatorTask.  `kind` is the `how` of `record_utils.join_records`."""
    keys: Sequence[Any]
    max_rows_per_record: int = 10_000
    kind: str = "inner"

    def task_name(self) -> str:
        return "join"


@dataclasses.dataclass
class OperatorInstanceConfig:
    """operator_handler_state.rs:28-35 (fields the tasks use)"""
    instance_id: int
    operator_id: str
    query_id: int
    task: Any
    device_id: int = 0


# ---- plugin API ------------------------------------------------------------------------------------------
class TaskBuilder(abc.ABC):
    """OPS/traits.rs:22-36.  `build` returns a callable that runs the task to completion and returns None on
    success or the error (the reference sends that through a oneshot channel)."""

    @abc.abstractmethod
    def build(self, op_in_config: OperatorInstanceConfig, inbound_exchanges: List[ExchangeOperator],
              outbound_exchange: Optional[ExchangeOperator]) -> Callable[[], Optional[Exception]]:
        ...


def _runner(task) -> Callable[[], Optional[Exception]]:
    """what every `TaskBuilder.build` returns: run `task` to completion; None, or the error that ended it.  The task is
    reachable as `run.task` (its counters are what the callers and the tests read)."""

    def run():
        try:
            task.async_main()
            return None
        except Exception as err:   # noqa: BLE001 -- any error ends the instance (producer_operator.rs:179-183)
            return err

    run.task = task
    return run


def _task_of(op_in_config: "OperatorInstanceConfig", task_type: type, a_name: str):
    """the operator task of `op_in_config`, which must be a `task_type` (`a_name`: "a filter", "an order by", ...)"""
    if not isinstance(op_in_config.task, task_type):
        raise ValueError(f"operator instance config is not {a_name} task")
    return op_in_config.task


def _max_rows_per_record(task) -> int:
    if task.max_rows_per_record < 1:
        raise ValueError("max_rows_per_record must be at least 1")
    return task.max_rows_per_record


class _LazyContext:
    """mixin of the tasks that call the library: `_ctx` is the context they were given, or the one `_context()` makes on
    the instance's device the first time the library is needed (never, when the compute functions are injected)"""
    _ctx = None

    def _context(self):
        if self._ctx is None:
            self._ctx = record_utils.Context(self.operator_instance_config.device_id)
        return self._ctx


class OperatorTaskRegistryError(Exception):
    pass


class OperatorTaskRegistry:
    # operator-task type -> (the attribute that holds its one builder, its name in the "already set" message)
    _SLOTS = {
        FilterOperatorTask: ("filter_task", "filter"),
        OrderByOperatorTask: ("order_by_task", "order by"),
        AggregateOperatorTask: ("aggregate_task", "aggregate"),
        JoinOperatorTask: ("join_task", "join"),
        WindowOperatorTask: ("window_task", "window"),
        MaterializeFilesOperatorTask: ("materialize_files_task", "materialize file"),
    }

    def __init__(self):
        self.filter_task: Optional[TaskBuilder] = None
        self.order_by_task: Optional[TaskBuilder] = None
        self.aggregate_task: Optional[TaskBuilder] = None
        self.join_task: Optional[TaskBuilder] = None
        self.window_task: Optional[TaskBuilder] = None
        self.materialize_files_task: Optional[TaskBuilder] = None
        self.materialize_data_formats: List[str] = []
        self.table_func_tasks: dict = {}

    def _set(self, task_type: type, builder: TaskBuilder) -> "OperatorTaskRegistry":
        """operator_task_registry.rs:51-57: exactly one builder per operator task"""
        slot, name = self._SLOTS[task_type]
        if getattr(self, slot) is not None:
            raise OperatorTaskRegistryError(f"{name} task builder already set")
        setattr(self, slot, builder)
        return self

    def add_filter_task_builder(self, builder: TaskBuilder) -> "OperatorTaskRegistry":
        return self._set(FilterOperatorTask, builder)

    def add_order_by_task_builder(self, builder: TaskBuilder) -> "OperatorTaskRegistry":
        return self._set(OrderByOperatorTask, builder)

    def add_aggregate_task_builder(self, builder: TaskBuilder) -> "OperatorTaskRegistry":
        return self._set(AggregateOperatorTask, builder)

    def add_window_task_builder(self, builder: TaskBuilder) -> "OperatorTaskRegistry":
        return self._set(WindowOperatorTask, builder)

    def add_join_task_builder(self, builder: TaskBuilder) -> "OperatorTaskRegistry":
        return self._set(JoinOperatorTask, builder)

    def add_materialize_files_builder(self, builder: TaskBuilder, data_formats: List[str]) -> "OperatorTaskRegistry":
        self._set(MaterializeFilesOperatorTask, builder)
        self.materialize_data_formats = list(data_formats)
        return self

    def add_table_func_task_builder(self, func_name: str, builder: TaskBuilder) -> "OperatorTaskRegistry":
        """operator_task_registry.rs:35-49 (the syntax validator is the planner's business: out of scope)"""
        if func_name in self.table_func_tasks:
            raise OperatorTaskRegistryError(f"table func task builder for {func_name} already set")
        self.table_func_tasks[func_name] = builder
        return self

    def find_task_builder(self, task) -> Optional[TaskBuilder]:
        if isinstance(task, ReadFilesOperatorTask):
            return self.table_func_tasks.get("read_files")
        if isinstance(task, MaterializeFilesOperatorTask) and task.data_format not in self.materialize_data_formats:
            return None
        for task_type, (slot, _) in self._SLOTS.items():
            if isinstance(task, task_type):
                return getattr(self, slot)
        return None


# ---- filter --------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class FilterConfig:
    expr: A.Expr

    @staticmethod
    def try_from(op_in_config: OperatorInstanceConfig) -> "FilterConfig":
        return FilterConfig(_task_of(op_in_config, FilterOperatorTask, "a filter").expr)


class FilterTask(_LazyContext):
    """filter_task.rs:65-142.  `group_size` > 1 is the GPU extension: the task drains up to that many queued records
    of one schema and filters them with ONE kernel launch (`record_utils.filter_records`); every output still
    carries its input record id and is acked individually, so the exchange protocol is unchanged."""

    def __init__(self, op_in_config: OperatorInstanceConfig, filter_config: FilterConfig,
                 inbound_exchanges, outbound_exchange, filter_fn=None, ctx=None, group_size: int = 1):
        self.operator_instance_config = op_in_config
        self.filter_config = filter_config
        self.inbound_exchanges = inbound_exchanges
        self.outbound_exchange = outbound_exchange
        self._filter = filter_fn
        self._ctx = ctx
        self.group_size = max(1, int(group_size))
        self.records_processed = 0
        self.rows_in = 0
        self.rows_out = 0
        self.group_calls = 0

    def _filter_record(self, rec, aliases):
        if self._filter is not None:
            return self._filter(rec, aliases, self.filter_config.expr)
        return record_utils.filter_record(rec, aliases, self.filter_config.expr, ctx=self._context())

    def _filter_group(self, group):
        """one library call for records that share schema, residency and table aliases; else record by record"""
        first = group[0]
        same = self._filter is None and len(group) > 1 and all(
            g.table_aliases == first.table_aliases and type(g.record) is type(first.record) and
            _schema_of(g.record) == _schema_of(first.record) for g in group[1:])
        if not same:
            return [self._filter_record(g.record, g.table_aliases) for g in group]
        self.group_calls += 1
        return record_utils.filter_records([g.record for g in group], first.table_aliases, self.filter_config.expr,
                                           ctx=self._context())

    def async_main(self) -> None:
        """filter_task.rs:65-142: pull -> filter -> push (same record id) -> ack"""
        rec_handler = RecordHandler.initiate(self.operator_instance_config, self.inbound_exchanges, self.outbound_exchange)
        try:   # an error ends the task (filter_task.rs `?`): its heartbeats must stop with it, so the exchange requeues
            while True:
                exchange_rec = rec_handler.next_record()
                if exchange_rec is None:
                    break
                group = [exchange_rec]
                while len(group) < self.group_size:
                    more = rec_handler.try_next_record()
                    if more is None:
                        break
                    group.append(more)
                for exchange_rec, filtered_rec in zip(group, self._filter_group(group)):
                    rec_handler.send_record_to_outbound_exchange(exchange_rec.record_id, filtered_rec, exchange_rec.table_aliases)
                    rec_handler.complete_record(exchange_rec)
                    self.records_processed += 1
                    self.rows_in += exchange_rec.record.num_rows
                    self.rows_out += filtered_rec.num_rows
        finally:
            rec_handler.close()


def _schema_of(rec):
    if hasattr(rec, "schema"):
        return rec.schema
    return tuple(zip(rec.column_names, rec.column_formats))


class FilterTaskBuilder(TaskBuilder):
    """The GPU filter operator. Swap it in with `OperatorTaskRegistry.add_filter_task_builder` -- the planner's
    DAG and the exchanges are untouched (operator_task_registry.rs:51-57)."""

    def __init__(self, filter_fn=None, group_size: int = 1):
        self._filter_fn = filter_fn
        self._group_size = group_size

    def build(self, op_in_config, inbound_exchanges, outbound_exchange):
        return _runner(FilterTask(op_in_config, FilterConfig.try_from(op_in_config), inbound_exchanges, outbound_exchange,
                                  filter_fn=self._filter_fn, group_size=self._group_size))


# ---- the blocking operators: order by, group by, window functions, join ----------------------------------------------
class BlockingTask(_LazyContext):
    """A blocking, single-instance operator: one that needs every input row before it can send the first output row.

    `async_main` is its whole protocol.  It pulls every record of every inbound side and holds them all (each tracked and
    heart-beaten by the side's RecordHandler meanwhile), hands them to `_compute` in ONE call, sends the result cut into
    records of at most `config.max_rows_per_record` rows with record ids 0, 1, 2, ... in result order -- a result without
    rows as one empty record, which carries the schema -- and only then acks its inputs: if the compute step or a send fails,
    nothing is acked, the handlers close, the heartbeats stop and the exchange requeues every input for another attempt
    (the ack-after-send rule of FilterTask, over the whole input instead of one record).  When a side delivered no record
    there is no schema to compute over: nothing is sent, and what the other sides delivered is acked.

    A subclass is a constructor and `_compute`.  `rows_in` counts the rows of every side, `rows_out` and `records_sent`
    what went out."""

    def __init__(self, op_in_config: OperatorInstanceConfig, config, inbound_exchanges, outbound_exchange, ctx=None):
        self.operator_instance_config = op_in_config
        self.config = config
        self.inbound_exchanges = inbound_exchanges
        self.outbound_exchange = outbound_exchange
        self._ctx = ctx
        self.rows_in = 0
        self.rows_out = 0
        self.records_sent = 0

    def _inbound_sides(self) -> List[list]:
        """the inbound exchanges of each side's RecordHandler.  One side, unless a subclass says otherwise (a handler reads
        only the first of its exchanges)."""
        return [self.inbound_exchanges]

    def _compute(self, *records_and_aliases):
        """-> (result, table aliases of the result's columns).  The arguments are, for each side in turn, the list of its
        records and the table aliases they came in under (those of the side's first record)."""
        raise NotImplementedError

    def async_main(self) -> None:
        handlers = [RecordHandler.initiate(self.operator_instance_config, exchanges, self.outbound_exchange)
                    for exchanges in self._inbound_sides()]
        try:
            held = [[] for _ in handlers]
            for handler, side in zip(handlers, held):
                while (exchange_rec := handler.next_record_to_hold()) is not None:
                    side.append(exchange_rec)
            self.rows_in = sum(h.record.num_rows for side in held for h in side)
            if all(held):
                args = []
                for side in held:
                    args += [[h.record for h in side], side[0].table_aliases]
                result, out_aliases = self._compute(*args)
                n, step = result.num_rows, self.config.max_rows_per_record
                # the first side's handler sends: they all share the outbound exchange
                for record_id, start in enumerate(range(0, max(n, 1), step)):
                    handlers[0].send_record_to_outbound_exchange(record_id, result.slice(start, min(step, n - start)), out_aliases)
                    self.records_sent += 1
                self.rows_out = n
            for handler, side in zip(handlers, held):   # every send is out: now, and only now, the inputs are done with
                for h in side:
                    handler.complete_record(h)
        finally:
            for handler in handlers:
                handler.close()


# ---- order by ---------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class OrderByConfig:
    order_by: Sequence[A.OrderByExpr]
    limit: Optional[int] = None
    max_rows_per_record: int = 10_000

    @staticmethod
    def try_from(op_in_config: OperatorInstanceConfig) -> "OrderByConfig":
        t = _task_of(op_in_config, OrderByOperatorTask, "an order by")
        if not t.order_by:
            raise ValueError("an order by task needs at least one key")
        return OrderByConfig(tuple(t.order_by), t.limit, _max_rows_per_record(t))


class OrderByTask(BlockingTask):
    """Sorts every inbound record with ONE `sort_records` call; the result goes out in sorted order under the table aliases
    of the input.  `sort_fn(records, table_aliases, order_by, limit)` replaces the library call (tests on the CPU)."""

    def __init__(self, op_in_config: OperatorInstanceConfig, config: OrderByConfig, inbound_exchanges, outbound_exchange,
                 sort_fn=None, ctx=None):
        super().__init__(op_in_config, config, inbound_exchanges, outbound_exchange, ctx)
        self._sort = sort_fn

    def _compute(self, records, aliases):
        c = self.config
        if self._sort is not None:
            return self._sort(records, aliases, c.order_by, c.limit), aliases
        return record_utils.sort_records(records, aliases, c.order_by, limit=c.limit, ctx=self._context()), aliases


class OrderByTaskBuilder(TaskBuilder):
    def __init__(self, sort_fn=None):
        self._sort_fn = sort_fn

    def build(self, op_in_config, inbound_exchanges, outbound_exchange):
        return _runner(OrderByTask(op_in_config, OrderByConfig.try_from(op_in_config), inbound_exchanges, outbound_exchange,
                                   sort_fn=self._sort_fn))


# ---- group by ---------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class AggregateConfig:
    keys: Sequence[A.Expr]
    items: Sequence[A.AggItem]
    max_rows_per_record: int = 10_000
    having: Optional[A.Expr] = None
    n_visible: Optional[int] = None

    @staticmethod
    def try_from(op_in_config: OperatorInstanceConfig) -> "AggregateConfig":
        t = _task_of(op_in_config, AggregateOperatorTask, "an aggregate")
        if not t.items:
            raise ValueError("an aggregate task needs at least one output item")
        if t.n_visible is not None and not 1 <= t.n_visible <= len(t.items):
            raise ValueError(f"an aggregate task shows 1 to {len(t.items)} of its items, not {t.n_visible}")
        return AggregateConfig(tuple(t.keys), tuple(t.items), _max_rows_per_record(t), t.having, t.n_visible)


def _no_aliases(record) -> List[list]:
    """table aliases of a record whose columns are new: no table prefix reaches them"""
    return [[] for _ in range(record.num_columns)]


class AggregateTask(BlockingTask):
    """Aggregates every inbound record with ONE `aggregate_records` call; the groups go out in key order, without table
    aliases.  When no record came in nothing is sent also without a GROUP BY key: there is no schema to aggregate over.
    HAVING is composition on that call's result: ONE `filter_record` with the predicate (a null drops the group), then,
    when hidden items stand behind the visible ones, ONE `project_record` to the first `n_visible` columns -- by position:
    visible items that share an output name aggregate under names of their own and get theirs back in the projection.
    `aggregate_fn(records, table_aliases, keys, items)`, `filter_fn(record, table_aliases, predicate)` and
    `project_fn(fields, record, table_aliases)` replace the library calls (tests on the CPU)."""

    def __init__(self, op_in_config: OperatorInstanceConfig, config: AggregateConfig, inbound_exchanges, outbound_exchange,
                 aggregate_fn=None, ctx=None, filter_fn=None, project_fn=None):
        super().__init__(op_in_config, config, inbound_exchanges, outbound_exchange, ctx)
        self._aggregate = aggregate_fn
        self._filter = filter_fn
        self._project = project_fn

    def _compute(self, records, aliases):
        c = self.config
        hidden = c.n_visible is not None and c.n_visible < len(c.items)
        items = list(c.items)
        if hidden:
            # The projection below names its columns, and a name resolves to the FIRST column that has it.  Visible items
            # that share an output name (`having_plan` never points the predicate at one of them) therefore aggregate
            # under names of their own, and the projection gives them their names back: the cut is positional.
            names = [it.name for it in items]
            taken = set(names)
            for i in range(c.n_visible):
                if names.count(names[i]) > 1:
                    k = i
                    while f"__visible_{k}" in taken:
                        k += 1
                    taken.add(f"__visible_{k}")
                    items[i] = dataclasses.replace(items[i], name=f"__visible_{k}")
        if self._aggregate is not None:
            result = self._aggregate(records, aliases, c.keys, tuple(items))
        else:
            result = record_utils.aggregate_records(records, aliases, c.keys, items, ctx=self._context())
        if c.having is not None:
            if self._filter is not None:
                result = self._filter(result, _no_aliases(result), c.having)
            else:
                result = record_utils.filter_record(result, _no_aliases(result), c.having, ctx=self._context())
        if hidden:
            fields = [A.UnnamedExpr(A.Identifier(A.Ident(it.name))) if it.name == orig.name else
                      A.ExprWithAlias(A.Identifier(A.Ident(it.name)), A.Ident(orig.name))
                      for it, orig in zip(items[:c.n_visible], c.items)]
            if self._project is not None:
                result = self._project(fields, result, _no_aliases(result))
            else:
                result = record_utils.project_record(fields, result, _no_aliases(result), ctx=self._context())
        return result, _no_aliases(result)


class AggregateTaskBuilder(TaskBuilder):
    def __init__(self, aggregate_fn=None, filter_fn=None, project_fn=None):
        self._aggregate_fn = aggregate_fn
        self._filter_fn = filter_fn
        self._project_fn = project_fn

    def build(self, op_in_config, inbound_exchanges, outbound_exchange):
        return _runner(AggregateTask(op_in_config, AggregateConfig.try_from(op_in_config), inbound_exchanges, outbound_exchange,
                                     aggregate_fn=self._aggregate_fn, filter_fn=self._filter_fn, project_fn=self._project_fn))


# ---- window functions -----------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class WindowConfig:
    partition_by: Sequence[A.Expr]
    order_by: Sequence[A.OrderByExpr]
    items: Sequence[A.WindowItem]
    projection: Sequence[A.SelectItem]
    max_rows_per_record: int = 10_000

    @staticmethod
    def try_from(op_in_config: OperatorInstanceConfig) -> "WindowConfig":
        t = _task_of(op_in_config, WindowOperatorTask, "a window")
        if not t.items:
            raise ValueError("a window task needs at least one item")
        if not t.projection:
            raise ValueError("a window task needs at least one projected field")
        return WindowConfig(tuple(t.partition_by), tuple(t.order_by), tuple(t.items), tuple(t.projection), _max_rows_per_record(t))


class WindowTask(BlockingTask):
    """Evaluates every window item with ONE `window_records` call over every inbound record (the rows come back in input
    order: record order, then row order) and finishes the SELECT list with ONE `project_record` over that result, which
    goes out without table aliases.  `window_fn(records, table_aliases, partition_by, order_by, items)` and
    `project_fn(fields, record, table_aliases)` replace the library calls (tests on the CPU)."""

    def __init__(self, op_in_config: OperatorInstanceConfig, config: WindowConfig, inbound_exchanges, outbound_exchange,
                 window_fn=None, project_fn=None, ctx=None):
        super().__init__(op_in_config, config, inbound_exchanges, outbound_exchange, ctx)
        self._window = window_fn
        self._project = project_fn

    def _compute(self, records, aliases):
        c = self.config
        if self._window is not None:
            windowed = self._window(records, aliases, c.partition_by, c.order_by, c.items)
        else:
            windowed = record_utils.window_records(records, aliases, c.partition_by, c.order_by, c.items, ctx=self._context())
        # the item columns are new: no table prefix reaches them
        win_aliases = None if aliases is None else list(aliases) + [[] for _ in range(windowed.num_columns - len(aliases))]
        if self._project is not None:
            result = self._project(c.projection, windowed, win_aliases)
        else:
            result = record_utils.project_record(c.projection, windowed, win_aliases, ctx=self._context())
        return result, _no_aliases(result)


class WindowTaskBuilder(TaskBuilder):
    def __init__(self, window_fn=None, project_fn=None):
        self._window_fn = window_fn
        self._project_fn = project_fn

    def build(self, op_in_config, inbound_exchanges, outbound_exchange):
        return _runner(WindowTask(op_in_config, WindowConfig.try_from(op_in_config), inbound_exchanges, outbound_exchange,
                                  window_fn=self._window_fn, project_fn=self._project_fn))


# ---- join ---------------------------------------------------------------------------------------------------------------
JOIN_KINDS = ("inner", "left", "right", "full", "semi", "anti")


@dataclasses.dataclass(frozen=True)
class JoinConfig:
    keys: Sequence[Any]
    max_rows_per_record: int = 10_000
    kind: str = "inner"

    @staticmethod
    def try_from(op_in_config: OperatorInstanceConfig) -> "JoinConfig":
        t = _task_of(op_in_config, JoinOperatorTask, "a join")
        if not t.keys:
            raise ValueError("a join task needs at least one pair of key columns")
        max_rows_per_record = _max_rows_per_record(t)
        if t.kind not in JOIN_KINDS:
            raise ValueError(f"a join task's kind must be one of {', '.join(JOIN_KINDS)}, not {t.kind!r}")
        return JoinConfig(tuple((l, r) for l, r in t.keys), max_rows_per_record, t.kind)


class JoinTask(BlockingTask):
    """The blocking protocol over TWO sides (inbound exchange 0: the left input, 1: the right): joins every record of both
    with ONE `join_records` call; the result goes out in the row order of its kind (inner: ascending by left row, then by
    right row) under the table aliases of the left columns followed by those of the right columns (semi and anti: the left
    columns only).  When either side delivered no record nothing is sent, whatever the kind: there is no schema to join or
    to pad with.
    Each side has a RecordHandler of its own: a handler reads only its first exchange and tracks by record id, which the two
    exchanges may share.
    `join_fn(left_records, left_aliases, right_records, right_aliases, keys)` replaces the library call (tests on the CPU);
    for a kind other than "inner" it is called with `kind=` as a keyword on top."""

    def __init__(self, op_in_config: OperatorInstanceConfig, config: JoinConfig, inbound_exchanges, outbound_exchange,
                 join_fn=None, ctx=None):
        if len(inbound_exchanges) != 2:
            raise ValueError(f"a join task takes two inbound exchanges (left, right), not {len(inbound_exchanges)}")
        super().__init__(op_in_config, config, inbound_exchanges, outbound_exchange, ctx)
        self._join = join_fn

    def _inbound_sides(self):
        return [[ex] for ex in self.inbound_exchanges]

    def _compute(self, left, left_aliases, right, right_aliases):
        c = self.config
        if self._join is None:
            result = record_utils.join_records(left, left_aliases, right, right_aliases, c.keys, ctx=self._context(), how=c.kind)
        elif c.kind == "inner":
            result = self._join(left, left_aliases, right, right_aliases, c.keys)
        else:
            result = self._join(left, left_aliases, right, right_aliases, c.keys, kind=c.kind)
        out_aliases = [list(a) for a in left_aliases]
        if c.kind not in ("semi", "anti"):
            out_aliases += [list(a) for a in right_aliases]
        return result, out_aliases


class JoinTaskBuilder(TaskBuilder):
    def __init__(self, join_fn=None):
        self._join_fn = join_fn

    def build(self, op_in_config, inbound_exchanges, outbound_exchange):
        return _runner(JoinTask(op_in_config, JoinConfig.try_from(op_in_config), inbound_exchanges, outbound_exchange,
                                join_fn=self._join_fn))


# ---- read_files (the table function in front of the path) -----------------------------------------------------
class ReadFilesTask(_LazyContext):
    """read_files_task.rs:129-291 with `read_records` (:233-282) on the GPU: every matching Parquet file is opened through a
    RANGE reader (the footer, then exactly the chunks that are decoded -- the reference reads through opendal ranges), its row
    groups are decoded in HBM (`chq_parquet_read_columns`) and forwarded as device-resident records cut into zero-copy slices
    of `max_rows_per_batch` rows; `columns` prunes the scan (the reference's DEV_NOTES.md:123).  Files the decoder refuses
    (status 30: ZSTD, nested columns, ...) are read with pyarrow on the host -- the stand-in for the parquet crate."""

    def __init__(self, op_in_config: OperatorInstanceConfig, task: ReadFilesOperatorTask, storage_root: str, outbound_exchange,
                 ctx=None, columns: Optional[Sequence[str]] = None, device_records: bool = True):
        self.operator_instance_config = op_in_config
        self.config = task
        self.storage_root = storage_root
        self.outbound_exchange = outbound_exchange
        self._ctx = ctx
        self.columns = list(columns) if columns is not None else None
        self.device_records = device_records
        self.record_id = 0
        self.files_read: List[str] = []
        self.bytes_fetched = 0
        self.host_fallbacks = 0

    def _send(self, rec_handler, record) -> None:
        aliases = record_utils.get_record_table_aliases(self.config.alias, record)
        rec_handler.send_record_to_outbound_exchange(self.record_id, record, aliases)
        self.record_id += 1

    def _read_records(self, rec_handler, path: str) -> None:
        size = os.path.getsize(path)
        step = max(1, int(self.config.max_rows_per_batch))
        with open(path, "rb") as fh:
            def read(offset: int, length: int) -> bytes:
                self.bytes_fetched += length
                return os.pread(fh.fileno(), length, offset)
            try:
                pf = record_utils.ParquetFile(None, reader=read, size=size)
            except record_utils.ChqError as err:
                if err.code != 30:
                    raise
                pf = None
            groups = None
            if pf is not None:
                try:
                    groups = pf.read_row_groups(ctx=self._context(), device_result=self.device_records, columns=self.columns)
                except record_utils.ChqError as err:
                    if err.code != 30:
                        raise
                finally:
                    pf.close()
        if groups is None:   # outside the GPU decoder's scope: the host reader, same batch size
            import pyarrow.parquet as pq
            self.host_fallbacks += 1
            for rec in pq.ParquetFile(path).iter_batches(batch_size=step, columns=self.columns):
                self._send(rec_handler, rec)
            return
        for group in groups:
            n = group.num_rows
            if n <= step:
                self._send(rec_handler, group)
                continue
            for at in range(0, n, step):
                self._send(rec_handler, group.slice(at, min(step, n - at)))

    def async_main(self) -> None:
        import glob
        rec_handler = RecordHandler.initiate(self.operator_instance_config, [], self.outbound_exchange)
        try:
            for path in sorted(glob.glob(os.path.join(self.storage_root, self.config.path.lstrip("/")), recursive=True)):
                self._read_records(rec_handler, path)
                self.files_read.append(path)
        finally:
            rec_handler.close()


class ReadFilesTaskBuilder(TaskBuilder):
    """The GPU read_files table function (`rust/gpu_read_files_task.rs` is the same task for the reference's registry)."""

    def __init__(self, storage_root: str, columns: Optional[Sequence[str]] = None, device_records: bool = True):
        self._root = storage_root
        self._columns = columns
        self._device_records = device_records

    def build(self, op_in_config, inbound_exchanges, outbound_exchange):
        task = _task_of(op_in_config, ReadFilesOperatorTask, "a read_files")
        return _runner(ReadFilesTask(op_in_config, task, self._root, outbound_exchange, columns=self._columns,
                                     device_records=self._device_records))


# ---- materialize ----------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class MaterializeFilesConfig:
    data_format: str
    fields: Sequence[A.SelectItem]

    @staticmethod
    def try_from(op_in_config: OperatorInstanceConfig) -> "MaterializeFilesConfig":
        t = _task_of(op_in_config, MaterializeFilesOperatorTask, "a materialize files")
        return MaterializeFilesConfig(t.data_format, t.fields)


class MaterializeFilesTask(_LazyContext):
    def __init__(self, op_in_config, config: MaterializeFilesConfig, inbound_exchanges, outbound_exchange,
                 storage_root: str, project_fn=None, ctx=None):
        self.operator_instance_config = op_in_config
        self.materialize_file_config = config
        self.inbound_exchanges = inbound_exchanges
        self.outbound_exchange = outbound_exchange
        self.storage_root = storage_root
        self._project = project_fn
        self._ctx = ctx
        self.files_written: List[str] = []

    def _project_record(self, rec, aliases):
        if self._project is not None:
            return self._project(self.materialize_file_config.fields, rec, aliases)
        # the projected batch stays in HBM: the Parquet pages are encoded there too
        return record_utils.project_record(self.materialize_file_config.fields, rec, aliases, ctx=self._context(), device_result=True)

    def _write_parquet(self, proj_rec, path: str) -> None:
        """materialize_files_task.rs:128-141 (AsyncArrowWriter ... write ... close).  A device-resident result is encoded on
        the GPU (`chq_record_to_parquet`) and only the finished file image reaches the host; column types that encoder does
        not write (and host-resident results, e.g. from an injected `project_fn`) go through pyarrow's writer."""
        import pyarrow as pa
        import pyarrow.parquet as pq
        if isinstance(proj_rec, record_utils.DeviceRecordBatch):
            try:
                image = record_utils.record_to_parquet(proj_rec, ctx=self._ctx, copy=False)
            except record_utils.ChqError as e:
                if e.code != 30:   # NotSupported: a type outside Int32/Int64/Float32/Float64/Boolean/Utf8
                    raise
                proj_rec = proj_rec.to_host()
            else:
                try:
                    with open(path, "wb") as f:
                        f.write(image.view)     # straight out of the library's host buffer
                finally:
                    image.release()
                return
        pq.write_table(pa.Table.from_batches([proj_rec]), path)

    def async_main(self) -> None:
        """materialize_files_task.rs:68-170: pull -> project -> write /query_results/<uuid>/rec_<id>.parquet -> ack."""
        rec_handler = RecordHandler.initiate(self.operator_instance_config, self.inbound_exchanges, self.outbound_exchange)
        query_uuid = uuid.UUID(int=self.operator_instance_config.query_id)
        out_dir = os.path.join(self.storage_root, "query_results", str(query_uuid))
        os.makedirs(out_dir, exist_ok=True)
        try:
            while True:
                exchange_rec = rec_handler.next_record()
                if exchange_rec is None:
                    break
                proj_rec = self._project_record(exchange_rec.record, exchange_rec.table_aliases)
                path = os.path.join(out_dir, f"rec_{exchange_rec.record_id}.parquet")
                self._write_parquet(proj_rec, path)
                self.files_written.append(path)
                rec_handler.complete_record(exchange_rec)
        finally:
            rec_handler.close()


class MaterializeFilesTaskBuilder(TaskBuilder):
    def __init__(self, storage_root: str, project_fn=None):
        self.storage_root = storage_root
        self._project_fn = project_fn

    def build(self, op_in_config, inbound_exchanges, outbound_exchange):
        return _runner(MaterializeFilesTask(op_in_config, MaterializeFilesConfig.try_from(op_in_config), inbound_exchanges,
                                            outbound_exchange, self.storage_root, project_fn=self._project_fn))


def build_default_operator_task_registry(storage_root: str) -> OperatorTaskRegistry:
    """operator_task_registry.rs:150-162 with the GPU builders swapped in."""
    return (OperatorTaskRegistry()
            .add_table_func_task_builder("read_files", ReadFilesTaskBuilder(storage_root))
            .add_filter_task_builder(FilterTaskBuilder())
            .add_order_by_task_builder(OrderByTaskBuilder())
            .add_aggregate_task_builder(AggregateTaskBuilder())
            .add_window_task_builder(WindowTaskBuilder())
            .add_join_task_builder(JoinTaskBuilder())
            .add_materialize_files_builder(MaterializeFilesTaskBuilder(storage_root), ["parquet"]))
